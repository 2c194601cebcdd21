// qt_gwa_gemm.hip -- packed group-wise affine weights (uintN / intN codes, one bf16 scale and zero point per block of `bs`
// consecutive k) and the Linear that reads them.
//
//   qt_gwa_pack              bf16 codes [N, K] -> packed bytes, once per weight (with the check the graph pass relies on)
//   qt_gwa_dequantize_bf16   packed codes + scale + zero point -> the bf16 weight [N, K], one pass
//   qt_linear_gwa_bf16       y[M, N] = x[M, K] . Wd[N, K]^T + bias with Wd = dequantize(codes) formed in registers
//
// Replaces, for a converted weight-only graph (quantize_pt2e._lower_group_wise_affine),
//     Wd = quantized_ops.dequantize(codes, scale, zero_point, (-1,), bs);  y = aten.linear(x, Wd, bias)
// which reads 2 bytes and writes 2 bytes per weight on every call before the GEMM reads the copy again.
//
// Packed layout (the kernels' own; pack_torch / unpack_torch in pt2e_native.py restate it).  Codes are stored as q - quant_min,
// 4 bits each when quant_max - quant_min <= 15, else 8.  The unit is what ONE WAVE feeds to v_mfma_f32_16x16x32_bf16 from one
// 16-byte load per lane: a 16-column group x one "super step" of 128 k (4 bits) or 64 k (8 bits) = 64 lanes x 16 bytes = 1 KiB,
//     piece(ng, ss, lane l = 16 g + r)  at byte ((ng * nss + ss) * 64 + l) * 16        nss = ceil(K / super step)
// and the lane's 16 bytes are its operand fragments of the super step's k steps j = 0 .. J-1 (J = 4 | 2), in order: the eight
// codes of column n = 16 ng + r at k = ss * 32 J + 32 j + 8 g + e, e = 0 .. 7 (4 bits: code e in nibble e of word j, low nibble
// first; 8 bits: byte e of the word pair j).  Columns beyond N and k beyond K hold code 0 and are never multiplied.
//
// The GEMM.  A wave owns one 16-column group and RT row tiles of 16 rows: per k step it turns its lane's eight codes into the
// eight bf16 values of dequantize -- gwa_dequant (qt_gwa.h), the very function of quantized_ops::dequantize's kernel -- and
// multiplies them with RT activation fragments read straight from global memory (they are small next to the weight and stay in
// the caches).  Operands are swapped (D rows = output columns) so that a lane ends up with four consecutive columns of one
// output row.  A lane reads the scale and the zero point of its column once per block (once per super step where a block spans
// several), together with the packed piece, a ring of kDepth super steps ahead of the multiplication.
// Row tiles are 16, 32 or 64 rows (RT = 1, 2, 4): the regime weight-only quantization exists for, bound by the packed weight's
// bytes.  A workgroup is 8 waves on ONE column group; they split K into 8 contiguous ranges of super steps, leave their fp32 sums
// in LDS, and waves 0 .. RT-1 add the eight partial sums IN RANGE ORDER: no atomics, no workspace, nothing to wait for, the
// same bits on every run.  More rows than a tile are further workgroups, each converting the weight again -- which is why the
// route rule (pt2e_native._gwa_route_takes) hands larger M to qt_gwa_dequantize_bf16 + the library GEMM (a 128-row
// variant of this register-only scheme was measured at 0.16 - 0.32 x that route's speed and is not shipped).
// fp32 accumulation in k order, bias added in fp32, one rounding to bf16.  No LDS beyond the partial sums, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_gwa.h"

namespace {

#pragma clang fp contract(off)

typedef short v8s __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

template <int BITS>
struct Geo {
    static constexpr int kJ = BITS == 4 ? 4 : 2;      // k steps (of 32) per super step
    static constexpr int kSK = 32 * kJ;               // k per super step
};
constexpr int kDepth = 4;                             // super steps a wave requests ahead

inline long gwa_nss(int K, int bits) { return bits == 4 ? (K + 127) / 128 : (K + 63) / 64; }
inline long gwa_pieces(int N, int K, int bits) { return (long)((N + 15) / 16) * gwa_nss(K, bits) * 64; }

// the eight codes of k step j of a lane's 16 bytes, as floats q = code + quant_min (exact)
template <int BITS>
__device__ __forceinline__ void piece_codes(const u32x4 &p, int j, float qmin, float (&q)[8]) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
    if constexpr (BITS == 4) {
        const uint32_t v = w[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (float)((v >> (4 * e)) & 15u) + qmin;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] = (float)((w[2 * j + (e >> 2)] >> (8 * (e & 3))) & 255u) + qmin;
    }
}

// ---- pack ------------------------------------------------------------------------------------------------------------------------
template <int BITS>
__global__ __launch_bounds__(256) void gwa_pack_kernel(const uint16_t *__restrict__ codes, u32x4 *__restrict__ packed, int N, int K,
                                                       int nss, long pieces, float qmin, float qmax, int *__restrict__ bad) {
    constexpr int J = Geo<BITS>::kJ, SK = Geo<BITS>::kSK;
    bool any_bad = false;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < pieces; p += (long)gridDim.x * 256) {
        const int l = (int)(p & 63), r = l & 15, g = l >> 4;
        const long t = p >> 6;
        const int ss = (int)(t % nss), n = (int)(t / nss) * 16 + r;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = ss * SK + j * 32 + g * 8;
            if (n >= N || k >= K) continue;                    // K % 32 == 0: a k step is inside K or outside
            const uint4 v = *(const uint4 *)(codes + (long)n * K + k);
            const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (e & 1) ? bf_hi(vw[e >> 1]) : bf_lo(vw[e >> 1]);
                const bool ok = (f == rintf(f)) & (f >= qmin) & (f <= qmax);       // NaN fails every comparison
                any_bad |= !ok;
                const uint32_t c = ok ? (uint32_t)(int)(f - qmin) : 0u;
                if constexpr (BITS == 4) w[j] |= c << (4 * e);
                else w[2 * j + (e >> 2)] |= c << (8 * (e & 3));
            }
        }
        packed[p] = u32x4{w[0], w[1], w[2], w[3]};
    }
    if (bad && any_bad) *bad = 1;                              // an ordinary vector store; every writer writes the same value
}

// ---- dequantize ------------------------------------------------------------------------------------------------------------------
// A wave's 64 pieces are 16 rows x one super step (256 or 128 bytes of bf16 per row), but a lane holds four (two) 16-byte runs of ITS
// row that are 64 bytes apart: stored from there, every store instruction would write half cache lines.  The wave turns its tile
// around in LDS and stores whole rows: lane l writes 16 bytes at (row i * rows-per-store + l / PR, position l % PR).
template <int BITS>
__global__ __launch_bounds__(256) void gwa_dequant_kernel(const u32x4 *__restrict__ packed, const uint16_t *__restrict__ scale,
                                                          const uint16_t *__restrict__ zp, uint16_t *__restrict__ y, int N, int K, int nss,
                                                          int bs_shift, long pieces, float qmin) {
    constexpr int J = Geo<BITS>::kJ, SK = Geo<BITS>::kSK;
    constexpr int PR = SK / 8;                       // 16-byte positions of a row of the tile
    constexpr int kRow = PR + 1;                     // (+ 1: rows 16 bytes further apart spread over the banks)
    __shared__ uint4 tile[4][16 * kRow];
    const int nkb = K >> bs_shift;
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6, r = l & 15, g = l >> 4;
    for (long base = (long)blockIdx.x * 256; base < pieces; base += (long)gridDim.x * 256) {      // uniform trip count: barriers inside
        const long p = base + threadIdx.x;
        const bool live = p < pieces;                // whole waves: pieces % 64 == 0
        const long t = p >> 6;
        const int ss = (int)(t % nss), n0 = (int)(t / nss) * 16;
        if (live) {
            const int n = min(n0 + r, N - 1);        // rows past N: clamped for reading, never stored
            const u32x4 pc = packed[p];
            float s = 0.f, z = 0.f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (j == 0 || ((j * 32) & ((1 << bs_shift) - 1)) == 0) {          // a new block starts here (uniform)
                    const long blk = (long)n * nkb + (min(ss * SK + j * 32, K - 32) >> bs_shift);
                    s = qt_bf2f(scale[blk]);
                    z = qt_bf2f(zp[blk]);
                }
                float q[8];
                piece_codes<BITS>(pc, j, qmin, q);
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = gwa_dequant<kIoBf16>(q[e], z, s);
                tile[w][r * kRow + j * 4 + g] = uint4{pack_bf16x2(q[0], q[1]), pack_bf16x2(q[2], q[3]), pack_bf16x2(q[4], q[5]), pack_bf16x2(q[6], q[7])};
            }
        }
        __syncthreads();
        if (live) {
#pragma unroll
            for (int i = 0; i < J; ++i) {
                const int row = i * (64 / PR) + l / PR, pos = l % PR;
                const int n = n0 + row, k = ss * SK + pos * 8;
                if (n < N && k < K) *(uint4 *)(y + (long)n * K + k) = tile[w][row * kRow + pos];
            }
        }
        __syncthreads();
    }
}

// ---- the GEMM --------------------------------------------------------------------------------------------------------------------
struct Args {
    const uint16_t *x;        // [M][K] bf16
    const u32x4 *packed;      // [n16][nss][64] pieces
    const uint16_t *scale;    // [N][K / bs] bf16
    const uint16_t *zp;       // [N][K / bs] bf16
    const uint16_t *bias;     // [N] bf16 or NULL
    uint16_t *y;              // [M][N] bf16
    int M, N, K;
    int nkb, bs, bs_shift;    // K / bs, bs, log2 bs
    int nss, n16, tiles_m;
    float qmin;
};

// RT: 16-row tiles of the workgroup's row tile.  Wave kw of the workgroup's kKW multiplies the kw-th of kKW contiguous ranges of super steps.
constexpr int kKW = 8;

template <int BITS, int RT>
__global__ __launch_bounds__(64 * kKW) void linear_gwa_kernel(Args a) {
    constexpr int J = Geo<BITS>::kJ, SK = Geo<BITS>::kSK, KW = kKW;
    static_assert(RT <= KW, "a wave per row tile adds the partial sums");
    __shared__ v4f red[KW * RT * 64];
    const int l = threadIdx.x & 63, kw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = l & 15, g = l >> 4;
    const int tm = blockIdx.x % a.tiles_m, ng = blockIdx.x / a.tiles_m;      // the row tiles of a column group are neighbours
    const int m0 = tm * 16 * RT;
    v4f acc[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) acc[i] = v4f{0.f, 0.f, 0.f, 0.f};
    {
        const int ss0 = (int)((long)kw * a.nss / KW), ss1 = (int)((long)(kw + 1) * a.nss / KW);
        // rows and columns past the end are clamped for READING (their products are never stored)
        const long nrow = min(ng * 16 + r, a.N - 1);
        const uint16_t *const srow = a.scale + nrow * a.nkb, *const zrow = a.zp + nrow * a.nkb;
        const u32x4 *const wp = a.packed + (long)ng * a.nss * 64 + l;
        const uint16_t *xr[RT];
#pragma unroll
        for (int i = 0; i < RT; ++i) xr[i] = a.x + (long)min(m0 + 16 * i + r, a.M - 1) * a.K + g * 8;

        u32x4 wq[kDepth];
        uint32_t sz[kDepth][J];                                              // scale (low half) and zero point of each k step
        auto request = [&](auto dc, int ss) __attribute__((always_inline)) {
            constexpr int d = decltype(dc)::value;
            wq[d] = wp[(long)ss * 64];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (j == 0 || ((j * 32) & (a.bs - 1)) == 0) {                // a new block starts here (uniform)
                    const int kb = min((ss * SK + j * 32) >> a.bs_shift, a.nkb - 1);      // (k steps beyond K: clamped, unused)
                    sz[d][j] = (uint32_t)srow[kb] | ((uint32_t)zrow[kb] << 16);
                } else {
                    sz[d][j] = sz[d][j - 1];
                }
            }
        };
        auto multiply = [&](auto dc, int ss) __attribute__((always_inline)) {
            constexpr int d = decltype(dc)::value;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int k = ss * SK + j * 32;
                if (k >= a.K) break;                                         // uniform: the ragged last super step
                u32x4 xa[RT];
#pragma unroll
                for (int i = 0; i < RT; ++i) xa[i] = *(const u32x4 *)(xr[i] + k);
                const float s = bf_lo(sz[d][j]), z = bf_hi(sz[d][j]);
                float q[8];
                piece_codes<BITS>(wq[d], j, a.qmin, q);
#pragma unroll
                for (int e = 0; e < 8; ++e) q[e] = gwa_dequant<kIoBf16>(q[e], z, s);
                const u32x4 wf = {pack_bf16x2(q[0], q[1]), pack_bf16x2(q[2], q[3]), pack_bf16x2(q[4], q[5]), pack_bf16x2(q[6], q[7])};
#pragma unroll
                for (int i = 0; i < RT; ++i)
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8s, wf), __builtin_bit_cast(v8s, xa[i]), acc[i], 0, 0, 0);
            }
        };
        auto slot = [&](auto dc, int ss) __attribute__((always_inline)) {
            constexpr int d = decltype(dc)::value;
            if (ss + d < ss1) {
                multiply(dc, ss + d);
                if (ss + d + kDepth < ss1) request(dc, ss + d + kDepth);
            }
        };
        if (ss0 + 0 < ss1) request(std::integral_constant<int, 0>{}, ss0 + 0);
        if (ss0 + 1 < ss1) request(std::integral_constant<int, 1>{}, ss0 + 1);
        if (ss0 + 2 < ss1) request(std::integral_constant<int, 2>{}, ss0 + 2);
        if (ss0 + 3 < ss1) request(std::integral_constant<int, 3>{}, ss0 + 3);
        static_assert(kDepth == 4, "the ring is written out for four slots");
        for (int ss = ss0; ss < ss1; ss += kDepth) {
            slot(std::integral_constant<int, 0>{}, ss);
            slot(std::integral_constant<int, 1>{}, ss);
            slot(std::integral_constant<int, 2>{}, ss);
            slot(std::integral_constant<int, 3>{}, ss);
        }
    }
    // lane (r, g) of row tile i holds y[m0 + 16 i + r][16 ng + 4 g .. + 3]
    auto store = [&](int i, v4f t) __attribute__((always_inline)) {
        const int row = m0 + 16 * i + r, col = ng * 16 + 4 * g;
        if (row < a.M && col < a.N) {                                        // N % 8 == 0: four columns are inside N or outside
            if (a.bias) {
                const uint2 b = *(const uint2 *)(a.bias + col);
                t[0] += bf_lo(b.x); t[1] += bf_hi(b.x); t[2] += bf_lo(b.y); t[3] += bf_hi(b.y);
            }
            *(uint2 *)(a.y + (long)row * a.N + col) = uint2{pack_bf16x2(t[0], t[1]), pack_bf16x2(t[2], t[3])};
        }
    };
#pragma unroll
    for (int i = 0; i < RT; ++i) red[(kw * RT + i) * 64 + l] = acc[i];
    __syncthreads();
    if (kw < RT) {                                                           // wave kw adds the partial sums of row tile kw
        v4f t = red[kw * 64 + l];
#pragma unroll
        for (int q = 1; q < KW; ++q) t += red[(q * RT + kw) * 64 + l];       // in range order, whoever finished first
        store(kw, t);
    }
}

template <int BITS, int RT>
int launch_gemm(const Args &a, hipStream_t st) {
    const long tiles = (long)a.tiles_m * a.n16;
    if (tiles > 0x7FFFFFFFL) return QT_ERR_BAD_ARG;
    linear_gwa_kernel<BITS, RT><<<(unsigned)tiles, 64 * kKW, 0, st>>>(a);
    return qt_launch_status();
}

template <int BITS>
int launch_tile(Args &a, int tile_m, hipStream_t st) {
    a.tiles_m = (a.M + tile_m - 1) / tile_m;
    switch (tile_m) {
        case 16: return launch_gemm<BITS, 1>(a, st);
        case 32: return launch_gemm<BITS, 2>(a, st);
        default: return launch_gemm<BITS, 4>(a, st);
    }
}

inline bool aligned(const void *p, uintptr_t n) { return (((uintptr_t)p) & (n - 1)) == 0; }

// log2 of a supported block size, or -1
inline int bs_shift_of(int bs) {
    switch (bs) {
        case 32: return 5;
        case 64: return 6;
        case 128: return 7;
        case 256: return 8;
        case 512: return 9;
        default: return -1;
    }
}

// what every entry point asks of the weight's shape
int shape_status(int N, int K, int bits) {
    if ((bits != 4 && bits != 8) || N < 1 || K < 1) return QT_ERR_BAD_ARG;
    if (K % 32 != 0 || N % 8 != 0) return QT_ERR_UNALIGNED;
    if ((long)N * K > (1L << 40)) return QT_ERR_BAD_ARG;
    return QT_OK;
}

}  // namespace

extern "C" {

size_t qt_gwa_packed_bytes(int N, int K, int bits) {
    if (shape_status(N, K, bits) != QT_OK) return 0;
    return (size_t)gwa_pieces(N, K, bits) * 16;
}

int qt_gwa_pack(const uint16_t *codes_dev, uint8_t *packed_dev, int N, int K, int bits, float quant_min, float quant_max, int *bad_dev,
                void *stream) {
    if (!codes_dev || !packed_dev) return QT_ERR_BAD_ARG;
    if (const int rc = shape_status(N, K, bits)) return rc;
    if (!(quant_max >= quant_min) || quant_max - quant_min > (bits == 4 ? 15.0f : 255.0f) || quant_min != rintf(quant_min) ||
        quant_max != rintf(quant_max))
        return QT_ERR_BAD_ARG;
    if (!aligned(codes_dev, 16) || !aligned(packed_dev, 16) || !aligned(bad_dev, 4)) return QT_ERR_UNALIGNED;
    const long pieces = gwa_pieces(N, K, bits);
    const int nss = (int)gwa_nss(K, bits);
    const unsigned grid = grid_for((size_t)pieces, 256, 16);
    hipStream_t st = (hipStream_t)stream;
    if (bits == 4) gwa_pack_kernel<4><<<grid, 256, 0, st>>>(codes_dev, (u32x4 *)packed_dev, N, K, nss, pieces, quant_min, quant_max, bad_dev);
    else gwa_pack_kernel<8><<<grid, 256, 0, st>>>(codes_dev, (u32x4 *)packed_dev, N, K, nss, pieces, quant_min, quant_max, bad_dev);
    return qt_launch_status();
}

int qt_gwa_dequantize_bf16(const uint8_t *packed_dev, const uint16_t *scale_dev, const uint16_t *zp_dev, uint16_t *y_dev, int N, int K,
                           int block_size, int bits, float quant_min, void *stream) {
    if (!packed_dev || !scale_dev || !zp_dev || !y_dev) return QT_ERR_BAD_ARG;
    if (const int rc = shape_status(N, K, bits)) return rc;
    const int shift = bs_shift_of(block_size);
    if (shift < 0) return QT_ERR_BAD_ARG;
    if (K % block_size != 0) return QT_ERR_UNALIGNED;
    if (!aligned(packed_dev, 16) || !aligned(y_dev, 16) || !aligned(scale_dev, 2) || !aligned(zp_dev, 2)) return QT_ERR_UNALIGNED;
    const long pieces = gwa_pieces(N, K, bits);
    const int nss = (int)gwa_nss(K, bits);
    const unsigned grid = grid_for((size_t)pieces, 256, 16);
    hipStream_t st = (hipStream_t)stream;
    if (bits == 4) gwa_dequant_kernel<4><<<grid, 256, 0, st>>>((const u32x4 *)packed_dev, scale_dev, zp_dev, y_dev, N, K, nss, shift, pieces, quant_min);
    else gwa_dequant_kernel<8><<<grid, 256, 0, st>>>((const u32x4 *)packed_dev, scale_dev, zp_dev, y_dev, N, K, nss, shift, pieces, quant_min);
    return qt_launch_status();
}

int qt_linear_gwa_tile(int M) { return M <= 16 ? 16 : M <= 32 ? 32 : 64; }

int qt_linear_gwa_bf16(const uint16_t *x_dev, const uint8_t *packed_dev, const uint16_t *scale_dev, const uint16_t *zp_dev,
                       const uint16_t *bias_dev, uint16_t *y_dev, int M, int N, int K, int block_size, int bits, float quant_min, int tile_m,
                       void *stream) {
    if (!x_dev || !packed_dev || !scale_dev || !zp_dev || !y_dev || M < 0) return QT_ERR_BAD_ARG;
    if (const int rc = shape_status(N, K, bits)) return rc;
    const int shift = bs_shift_of(block_size);
    if (shift < 0 || !(tile_m == 0 || tile_m == 16 || tile_m == 32 || tile_m == 64)) return QT_ERR_BAD_ARG;
    if (K % block_size != 0) return QT_ERR_UNALIGNED;
    if ((long)M * K > (1L << 40) || (long)M * N > (1L << 40)) return QT_ERR_BAD_ARG;
    if (!aligned(x_dev, 16) || !aligned(packed_dev, 16) || !aligned(y_dev, 16) || !aligned(scale_dev, 2) || !aligned(zp_dev, 2) ||
        !aligned(bias_dev, 8))
        return QT_ERR_UNALIGNED;
    if (M == 0) return QT_OK;
    Args a{};
    a.x = x_dev; a.packed = (const u32x4 *)packed_dev; a.scale = scale_dev; a.zp = zp_dev; a.bias = bias_dev; a.y = y_dev;
    a.M = M; a.N = N; a.K = K;
    a.nkb = K / block_size; a.bs = block_size; a.bs_shift = shift;
    a.nss = (int)gwa_nss(K, bits); a.n16 = (N + 15) / 16;
    a.qmin = quant_min;
    if (tile_m == 0) tile_m = qt_linear_gwa_tile(M);
    hipStream_t st = (hipStream_t)stream;
    return bits == 4 ? launch_tile<4>(a, tile_m, st) : launch_tile<8>(a, tile_m, st);
}

}  // extern "C"
