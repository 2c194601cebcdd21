// qt_groupwise.hip -- group-wise affine quantization (qs=group_wise_affine): one scale and one zero point per block of `bs`
// consecutive indices of one axis.
//
//   qt_fake_quant_gwa_*      GroupWiseAffineFakeQuantFunction.forward              (fake_quantize.py:136-194)
//   qt_quantize_blocks_*     quantized_ops::quantize with block-wise scale + zero point   (decomposed.py:173-210)
//   qt_dequantize_blocks_*   quantized_ops::dequantize with block-wise scale + zero point (decomposed.py:220-262)
//
// Every family sees the tensor as contiguous [outer][n][inner]; blocks are bs consecutive indices of n and the block parameters
// are [outer][n / bs][inner] in the tensor's dtype.  inner == 1 is the last-axis layout (a block is adjacent memory, handled like
// fq_mx_kernel: a block is bs/8 (bf16) or bs/4 (fp32) adjacent lanes of one wave); inner > 1 is the strided layout (ax=-2 on
// [B, H, S, D]: outer = B H, n = S, inner = D), where a lane owns one 16-byte piece of a row and walks rows of its block.
//
// The arithmetic is the torch composite's, operation for operation: for bf16 every step is computed in fp32 and rounded to bf16,
// for fp32 there is no intermediate rounding.  Each element is read once and written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_device.h"
#include "qt_chain.h"
#include "qt_gwa.h"

namespace {

// a * b + c must stay two roundings everywhere in this file
#pragma clang fp contract(off)

template <int IO>
constexpr int kPerVec = IO == kIoBf16 ? 8 : 4;               // elements of one 16-byte vector

// torch.amin / amax: NaN on either side wins
__device__ __forceinline__ float nan_min(float a, float b) { return ((b < a) | (b != b)) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return ((b > a) | (b != b)) ? b : a; }

template <int IO>
__device__ __forceinline__ float map_io(const uint16_t *__restrict__ t, float f) {      // quantized_ops::vmap, table in global memory
    const uint32_t img = IO == kIoBf16 ? qt_f2u(f) : qt_fold_img(qt_f2u(f));
    return qt_bf2f(t[img >> 16]);
}

// torch.clamp: min(max(q, lo), hi) in std::max / std::min operand order (keeps NaN and -0)
__device__ __forceinline__ float clamp_keep(float q, float lo, float hi) {
    q = q < lo ? lo : q;
    return q > hi ? hi : q;
}

template <int IO>
__device__ __forceinline__ void unpack_vec(const uint4 v, float (&f)[kPerVec<IO>]) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (IO == kIoBf16) {
            f[2 * j] = bf_lo(w[j]);
            f[2 * j + 1] = bf_hi(w[j]);
        } else {
            f[j] = qt_u2f(w[j]);
        }
    }
}

// values that are exact in the tensor's dtype -> one 16-byte vector
template <int IO>
__device__ __forceinline__ uint4 pack_vec(const float (&f)[kPerVec<IO>]) {
    if constexpr (IO == kIoBf16)
        return uint4{pack_bf16x2(f[0], f[1]), pack_bf16x2(f[2], f[3]), pack_bf16x2(f[4], f[5]), pack_bf16x2(f[6], f[7])};
    else
        return uint4{qt_f2u(f[0]), qt_f2u(f[1]), qt_f2u(f[2]), qt_f2u(f[3])};
}

struct GwaRange {
    float qmin, qmax, span;      // span = quant_max - quant_min in the tensor's dtype
};

// Scale and zero point of one block from its min and max (fake_quantize.py:166-182).
template <int IO>
__device__ __forceinline__ void gwa_params(float lo, float hi, const GwaRange &q, const uint16_t *__restrict__ scale_lut, float &sf,
                                           float &zp) {
    sf = rd_io<IO>(rd_io<IO>(hi - lo) / q.span);
    sf = sf > 0.0f ? sf : 1.0f;                               // constant blocks, and NaN
    zp = rd_io<IO>(rd_io<IO>(-lo / sf) + q.qmin);             // -lo is exact
    if (scale_lut) {                                          // after BOTH are computed
        sf = map_io<IO>(scale_lut, sf);
        zp = map_io<IO>(scale_lut, zp);
    }
}

// One 16-byte vector: y = (clamp(rint(x / sf + zp), qmin, qmax) - zp) * sf.  NP == 1: one (sf, zp) for the whole vector;
// NP == elements per vector: one per column.  FAST (bf16 only): x * (1 / sf) under UniformDiv's contract -- the quotient feeds
// a bf16 rounding -- and `bad` tells the caller to redo the vector with the IEEE division.
template <int IO, int NP, bool FAST>
__device__ __forceinline__ uint4 gwa_vec_d(const uint4 in, const UniformDiv (&dv)[NP], const float (&zp)[NP], const GwaRange &q, bool &bad) {
    const uint32_t w[4] = {in.x, in.y, in.z, in.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (IO == kIoBf16) {
            const UniformDiv &d0 = dv[NP == 1 ? 0 : 2 * j], &d1 = dv[NP == 1 ? 0 : 2 * j + 1];
            const float z0 = zp[NP == 1 ? 0 : 2 * j], z1 = zp[NP == 1 ? 0 : 2 * j + 1];
            const float x0 = bf_lo(w[j]), x1 = bf_hi(w[j]);
            uint32_t t;
            if constexpr (FAST) t = pack_bf16x2(d0.fast16(x0, bad), d1.fast16(x1, bad));
            else t = pack_bf16x2(d0.exact(x0), d1.exact(x1));
            t = pack_bf16x2(bf_lo(t) + z0, bf_hi(t) + z1);
            const float r0 = clamp_keep(rintf(bf_lo(t)), q.qmin, q.qmax), r1 = clamp_keep(rintf(bf_hi(t)), q.qmin, q.qmax);
            t = pack_bf16x2(r0 - z0, r1 - z1);
            o[j] = pack_bf16x2(bf_lo(t) * d0.s, bf_hi(t) * d1.s);
        } else {
            const UniformDiv &d = dv[NP == 1 ? 0 : j];
            const float z = zp[NP == 1 ? 0 : j];
            const float r = clamp_keep(rintf(d.exact(qt_u2f(w[j])) + z), q.qmin, q.qmax);
            o[j] = qt_f2u((r - z) * d.s);
        }
    }
    return uint4{o[0], o[1], o[2], o[3]};
}

template <int IO, int NP>
__device__ __forceinline__ uint4 gwa_vec(const uint4 in, const UniformDiv (&dv)[NP], const float (&zp)[NP], const GwaRange &q) {
    bool bad = false;
    if constexpr (IO == kIoBf16) {
        bool safe = true;
#pragma unroll
        for (int c = 0; c < NP; ++c) safe &= dv[c].safe;
        if (safe) {
            const uint4 r = gwa_vec_d<IO, NP, true>(in, dv, zp, q, bad);
            if (!bad) return r;
        }
    }
    return gwa_vec_d<IO, NP, false>(in, dv, zp, q, bad);
}

// ---- fake-quant, last-axis layout: grid-stride over 16-byte vectors, block min / max by sub-wave shuffles ----------------------
constexpr int kGwaLastBlocksPerCu = 8;      // 8 x 4 waves fill a CU; the grid loop takes the rest

template <int IO>
__global__ __launch_bounds__(256) void fq_gwa_last_kernel(const uint4 *__restrict__ x, uint4 *__restrict__ y, void *__restrict__ sf_out,
                                                          void *__restrict__ zp_out, size_t nvec, int group, GwaRange q,
                                                          const uint16_t *__restrict__ scale_lut) {
    constexpr int K = kPerVec<IO>;
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t iters = (nvec + stride - 1) / stride;
    for (size_t it = 0; it < iters; ++it) {
        const size_t v = it * stride + (size_t)blockIdx.x * 256 + threadIdx.x;
        const bool live = v < nvec;                           // nvec % group == 0: a block's lanes are all live or all idle
        uint4 in = {0u, 0u, 0u, 0u};
        if (live) in = x[v];
        float f[K];
        unpack_vec<IO>(in, f);
        float lo = f[0], hi = f[0];
#pragma unroll
        for (int j = 1; j < K; ++j) {
            lo = nan_min(lo, f[j]);
            hi = nan_max(hi, f[j]);
        }
        for (int off = 1; off < group; off <<= 1) {           // block min / max over `group` adjacent lanes
            lo = nan_min(lo, __shfl_xor(lo, off, 64));
            hi = nan_max(hi, __shfl_xor(hi, off, 64));
        }
        float sf, zp;
        gwa_params<IO>(lo, hi, q, scale_lut, sf, zp);
        if (live && (threadIdx.x & (group - 1)) == 0) {
            const size_t blk = v / (size_t)group;
            if constexpr (IO == kIoBf16) {
                ((uint16_t *)sf_out)[blk] = (uint16_t)(qt_f2u(sf) >> 16);
                ((uint16_t *)zp_out)[blk] = (uint16_t)(qt_f2u(zp) >> 16);
            } else {
                ((float *)sf_out)[blk] = sf;
                ((float *)zp_out)[blk] = zp;
            }
        }
        const UniformDiv dv[1] = {UniformDiv(sf)};
        const float z[1] = {zp};
        const uint4 r = gwa_vec<IO, 1>(in, dv, z, q);
        if (live) y[v] = r;
    }
}

// ---- fake-quant, strided layout ----------------------------------------------------------------------------------------------------
// A work item is one 16-byte column piece of one block: item m = (block, piece), pieces fastest, so consecutive lanes read
// consecutive pieces of a row.  A 256-thread workgroup is [G row groups][C = 256 / G items]; row group g keeps rows
// [g R, (g + 1) R) of the block in registers (R <= kGwaRows), the G partial minima / maxima of an item meet in LDS, and every
// thread then quantizes the rows it holds: one read and one write of the tensor, whatever bs.  The parameters of item m are
// the m-th 16-byte vector of scale / zero_point ([outer][n / bs][inner]).
constexpr int kGwaRows = 8;

template <int IO>
__global__ __launch_bounds__(256) void fq_gwa_strided_kernel(const uint4 *__restrict__ x, uint4 *__restrict__ y, uint4 *__restrict__ sf_out,
                                                             uint4 *__restrict__ zp_out, size_t items, uint32_t P, int bs, int G, int R,
                                                             GwaRange q, const uint16_t *__restrict__ scale_lut) {
    constexpr int K = kPerVec<IO>;
    __shared__ uint4 part[2][256];
    const int C = 256 / G;
    const int c = threadIdx.x & (C - 1), g = threadIdx.x / C;
    const size_t m = (size_t)blockIdx.x * C + c;
    const bool live = m < items;
    const size_t blk = m / P;
    const size_t base = blk * (size_t)bs * P + (m - blk * P);        // vector index of row 0 of the block, this piece
    const int r0 = g * R;
    const int nrows = live ? min(R, bs - r0) : 0;                     // may be <= 0 in the last row groups
    const uint4 *xr = x + base + (size_t)r0 * P;
    uint4 d[kGwaRows];
#pragma unroll
    for (int j = 0; j < kGwaRows; ++j)
        if (j < nrows) d[j] = xr[(size_t)j * P];
    float lo[K], hi[K];
#pragma unroll
    for (int e = 0; e < K; ++e) {
        lo[e] = qt_u2f(0x7F800000u);
        hi[e] = qt_u2f(0xFF800000u);
    }
#pragma unroll
    for (int j = 0; j < kGwaRows; ++j) {
        if (j < nrows) {
            float f[K];
            unpack_vec<IO>(d[j], f);
#pragma unroll
            for (int e = 0; e < K; ++e) {
                lo[e] = nan_min(lo[e], f[e]);
                hi[e] = nan_max(hi[e], f[e]);
            }
        }
    }
    if (G > 1) {                                                      // uniform: the partial results of the G row groups meet in LDS
        part[0][threadIdx.x] = pack_vec<IO>(lo);
        part[1][threadIdx.x] = pack_vec<IO>(hi);
        __syncthreads();
        for (int gg = 0; gg < G; ++gg) {
            if (gg == g) continue;
            float a[K], b[K];
            unpack_vec<IO>(part[0][gg * C + c], a);
            unpack_vec<IO>(part[1][gg * C + c], b);
#pragma unroll
            for (int e = 0; e < K; ++e) {
                lo[e] = nan_min(lo[e], a[e]);
                hi[e] = nan_max(hi[e], b[e]);
            }
        }
    }
    UniformDiv dv[K];
    float sf[K], zp[K];
#pragma unroll
    for (int e = 0; e < K; ++e) {
        gwa_params<IO>(lo[e], hi[e], q, scale_lut, sf[e], zp[e]);
        dv[e] = UniformDiv(sf[e]);
    }
    if (live && g == 0) {
        sf_out[m] = pack_vec<IO>(sf);
        zp_out[m] = pack_vec<IO>(zp);
    }
    uint4 *yr = y + base + (size_t)r0 * P;
#pragma unroll
    for (int j = 0; j < kGwaRows; ++j)
        if (j < nrows) yr[(size_t)j * P] = gwa_vec<IO, K>(d[j], dv, zp, q);
}

// ---- quantize / dequantize with block-wise scale and zero point ---------------------------------------------------------------------
// MODE 0: y = map[x / s + z]; MODE 1: y = out_map?[(in_map?[x] - z) * s].  STRIDED: the parameters of a vector are one 16-byte vector
// (one per column); otherwise one element for the whole vector.  `unit` = vectors per block of the last-axis layout, or rows per
// block of the strided one.
template <int IO, int MODE, bool STRIDED>
__global__ __launch_bounds__(256) void qdq_blocks_kernel(const uint4 *__restrict__ x, uint4 *__restrict__ y, const void *__restrict__ scale,
                                                         const void *__restrict__ zero_point, size_t nvec, uint32_t P, uint32_t unit,
                                                         const uint16_t *__restrict__ in_lut, const uint16_t *__restrict__ out_lut) {
    constexpr int K = kPerVec<IO>;
    for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (size_t)gridDim.x * 256) {
        float s[K], z[K], f[K];
        if constexpr (STRIDED) {
            const size_t row = v / P, pv = (row / unit) * P + (v - row * P);
            unpack_vec<IO>(((const uint4 *)scale)[pv], s);
            unpack_vec<IO>(((const uint4 *)zero_point)[pv], z);
        } else {
            const size_t blk = v / unit;
            float s0, z0;
            if constexpr (IO == kIoBf16) {
                s0 = qt_bf2f(((const uint16_t *)scale)[blk]);
                z0 = qt_bf2f(((const uint16_t *)zero_point)[blk]);
            } else {
                s0 = ((const float *)scale)[blk];
                z0 = ((const float *)zero_point)[blk];
            }
#pragma unroll
            for (int e = 0; e < K; ++e) {
                s[e] = s0;
                z[e] = z0;
            }
        }
        unpack_vec<IO>(x[v], f);
#pragma unroll
        for (int e = 0; e < K; ++e) {
            if constexpr (MODE == 0) {
                f[e] = map_io<IO>(out_lut, rd_io<IO>(rd_io<IO>(f[e] / s[e]) + z[e]));
            } else {
                if (in_lut) f[e] = map_io<IO>(in_lut, f[e]);
                f[e] = gwa_dequant<IO>(f[e], z[e], s[e]);
                if (out_lut) f[e] = map_io<IO>(out_lut, f[e]);
            }
        }
        y[v] = pack_vec<IO>(f);
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------------
inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// The layout rules shared by the three families; QT_OK when the kernels take the view.
template <int IO>
int gwa_view_status(size_t n, size_t inner, int bs) {
    constexpr int K = kPerVec<IO>;
    if (inner == 1) {
        if (bs < K || (bs & (bs - 1)) || bs > 64 * K) return QT_ERR_BAD_ARG;
    } else {
        if (bs < 1 || bs > 512) return QT_ERR_BAD_ARG;
        if (inner % K) return QT_ERR_UNALIGNED;
        if (inner / K > 0xFFFFFFFFull) return QT_ERR_BAD_ARG;
    }
    return n % (size_t)bs ? QT_ERR_UNALIGNED : QT_OK;          // the composite zero-pads, and the pad takes part in min / max
}

template <int IO>
int launch_gwa(const void *x, void *y, void *sf, void *zp, size_t outer, size_t n, size_t inner, int bs, float quant_min, float quant_max,
               const uint16_t *scale_lut, void *stream) {
    if (outer * n * inner == 0) return QT_OK;
    if (!x || !y || !sf || !zp) return QT_ERR_BAD_ARG;
    if (const int rc = gwa_view_status<IO>(n, inner, bs)) return rc;
    if (!aligned16(x) || !aligned16(y) || !aligned16(sf) || !aligned16(zp)) return QT_ERR_UNALIGNED;
    if (!(quant_max > quant_min)) return QT_ERR_BAD_ARG;
    constexpr int K = kPerVec<IO>;
    GwaRange q{quant_min, quant_max, quant_max - quant_min};
    if constexpr (IO == kIoBf16) q.span = qt_bf2f(qt_f2bf(q.span));
    hipStream_t st = (hipStream_t)stream;
    if (inner == 1) {
        const size_t nvec = outer * n / K;
        fq_gwa_last_kernel<IO><<<grid_for(nvec, 256, kGwaLastBlocksPerCu), 256, 0, st>>>((const uint4 *)x, (uint4 *)y, sf, zp, nvec, bs / K, q,
                                                                                         scale_lut);
    } else {
        int G = 1;
        while (G * kGwaRows < bs) G <<= 1;                     // 1 .. 64 row groups
        const int R = (bs + G - 1) / G, C = 256 / G;
        const uint32_t P = (uint32_t)(inner / K);
        const size_t items = outer * (n / (size_t)bs) * P;
        const size_t grid = (items + C - 1) / C;
        if (grid > 0x7FFFFFFFull) return QT_ERR_BAD_ARG;
        fq_gwa_strided_kernel<IO><<<(unsigned)grid, 256, 0, st>>>((const uint4 *)x, (uint4 *)y, (uint4 *)sf, (uint4 *)zp, items, P, bs, G, R, q,
                                                                  scale_lut);
    }
    return qt_launch_status();
}

template <int IO, int MODE>
int launch_qdq_blocks(const void *x, void *y, const void *scale, const void *zp, size_t outer, size_t n, size_t inner, int bs,
                      const uint16_t *in_lut, const uint16_t *out_lut, void *stream) {
    if (outer * n * inner == 0) return QT_OK;
    if (!x || !y || !scale || !zp || (MODE == 0 && !out_lut)) return QT_ERR_BAD_ARG;
    if (const int rc = gwa_view_status<IO>(n, inner, bs)) return rc;
    if (!aligned16(x) || !aligned16(y) || !aligned16(scale) || !aligned16(zp)) return QT_ERR_UNALIGNED;
    constexpr int K = kPerVec<IO>;
    const size_t nvec = outer * n * inner / K;
    const unsigned grid = grid_for(nvec, 256, 16);
    hipStream_t st = (hipStream_t)stream;
    if (inner == 1)
        qdq_blocks_kernel<IO, MODE, false><<<grid, 256, 0, st>>>((const uint4 *)x, (uint4 *)y, scale, zp, nvec, 1u, (uint32_t)(bs / K), in_lut, out_lut);
    else
        qdq_blocks_kernel<IO, MODE, true><<<grid, 256, 0, st>>>((const uint4 *)x, (uint4 *)y, scale, zp, nvec, (uint32_t)(inner / K), (uint32_t)bs, in_lut,
                                                                out_lut);
    return qt_launch_status();
}

}  // namespace

extern "C" {

int qt_fake_quant_gwa_bf16(const uint16_t *x, uint16_t *y, uint16_t *scale_out, uint16_t *zp_out, size_t outer, size_t n, size_t inner,
                           int block_size, float quant_min, float quant_max, const uint16_t *scale_lut, void *stream) {
    return launch_gwa<kIoBf16>(x, y, scale_out, zp_out, outer, n, inner, block_size, quant_min, quant_max, scale_lut, stream);
}
int qt_fake_quant_gwa_f32(const float *x, float *y, float *scale_out, float *zp_out, size_t outer, size_t n, size_t inner, int block_size,
                          float quant_min, float quant_max, const uint16_t *scale_lut, void *stream) {
    return launch_gwa<kIoF32>(x, y, scale_out, zp_out, outer, n, inner, block_size, quant_min, quant_max, scale_lut, stream);
}

int qt_quantize_blocks_bf16(const uint16_t *x, uint16_t *y, const uint16_t *scale, const uint16_t *zero_point, size_t outer, size_t n,
                            size_t inner, int block_size, const uint16_t *lut, void *stream) {
    return launch_qdq_blocks<kIoBf16, 0>(x, y, scale, zero_point, outer, n, inner, block_size, nullptr, lut, stream);
}
int qt_quantize_blocks_f32(const float *x, float *y, const float *scale, const float *zero_point, size_t outer, size_t n, size_t inner,
                           int block_size, const uint16_t *lut, void *stream) {
    return launch_qdq_blocks<kIoF32, 0>(x, y, scale, zero_point, outer, n, inner, block_size, nullptr, lut, stream);
}

int qt_dequantize_blocks_bf16(const uint16_t *x, uint16_t *y, const uint16_t *scale, const uint16_t *zero_point, size_t outer, size_t n,
                              size_t inner, int block_size, const uint16_t *in_lut, const uint16_t *out_lut, void *stream) {
    return launch_qdq_blocks<kIoBf16, 1>(x, y, scale, zero_point, outer, n, inner, block_size, in_lut, out_lut, stream);
}
int qt_dequantize_blocks_f32(const float *x, float *y, const float *scale, const float *zero_point, size_t outer, size_t n, size_t inner,
                             int block_size, const uint16_t *in_lut, const uint16_t *out_lut, void *stream) {
    return launch_qdq_blocks<kIoF32, 1>(x, y, scale, zero_point, outer, n, inner, block_size, in_lut, out_lut, stream);
}

}  // extern "C"
