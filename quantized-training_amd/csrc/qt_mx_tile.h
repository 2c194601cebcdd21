// qt_mx_tile.h -- what the kernels on 128-deep k tiles of packed codes share: the launch arguments, the matrix step (Mma), the LDS
// image of an operand tile and its fragment read (Tile, read_frag), the workgroup-id -> tile map, the dense register-staged operand
// side (DenseSide), the multiplication of one staged k tile (mma_tile), and the epilogues: values (emit_tile) or the next
// convolution's codes (emit_codes_tile).
// Used by qt_mx_gemm.hip (block-scaled float GEMM and the int8 GEMM on its kernels), qt_mx_conv.hip (conv2d_mx / conv2d_q as implicit
// GEMMs, depthwise conv2d_q) and qt_mxi_gemm.hip (integer / codebook operands under any block scale).
//
// Operand memory layout ("packed MX operand"): codes[rows][K * bits / 8] row-major, K contiguous, element i of a row
// in bits [i*bits, (i+1)*bits) little-endian; scales[rows][K / 32] E8M0 bytes (2^(byte - 127)).
// Fragment layout of the instruction (measured, tools/probe_mx_mfma*.hip): lane l = (row r = l & 15, group g = l >> 4)
//   fp6 / fp4: k = 32 g + [0, 32) of the 128-deep step;   fp8: bytes 0-15 <- k = 16 g + [0, 16), bytes 16-31 <- k = 64 + 16 g + [0, 16)
//   scale register byte 0 of lane (r, g) = scale of row r, k in [32 g, 32 g + 32);   D: col = l & 15, row = 4 (l >> 4) + i.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_dispatch.h"
#include "qt_formats.h"
#include "qt_mx.h"
#include "qt_qdq.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBM = 128, kBN = 128, kBK = 128;      // block tile (elements)

__host__ __device__ constexpr int tile_row_bytes(int f) { return f < 2 ? 128 : (f < 4 ? 96 : 64); }
using qt_mx::elem_bits;

struct MxGemmArgs {
    const uint8_t *A, *B;        // packed codes [batch][M][K*bitsA/8], [batch][N][K*bitsB/8]
    const uint8_t *sA, *sB;      // E8M0 [batch][M][K/32], [batch][N][K/32]
    void *C;                     // [batch][M][N] bf16 or f32
    const void *bias;            // [N] in C's dtype, or NULL
    int M, N, K;
    long bA, bB, bsA, bsB, bC;   // batch strides: bytes for A / B / scales, elements for C
    int out_f32;
    const void *out_scale;       // I8 kernels: dequantize factor(s) in C's dtype applied after the rounding of (acc + bias), or NULL
    int out_scale_per_col;       // 0: one factor, 1: one per output column
    int out_fold_f32;            // fp32 output: pass (acc + bias) through the identity value map first (hi16 | sticky, decomposed.py:151-153)
};

typedef int v4i __attribute__((ext_vector_type(4)));

// One 128-deep step of a 16 x 16 output tile.  I8: both operands are int8 codes (same tile layout as the 8-bit float
// formats: a lane's bytes 0-15 are k = 16 g + [0, 16) of the first 64-deep half, bytes 16-31 the same of the second), two
// v_mfma_i32_16x16x64_i8 with exact int32 accumulation; otherwise the block-scaled float instruction.
template <int FA, int FB, bool I8>
struct Mma {
    using acc_t = std::conditional_t<I8, v4i, v4f>;
    static __device__ __forceinline__ acc_t zero() {
        if constexpr (I8) return v4i{0, 0, 0, 0};
        else return v4f{0.f, 0.f, 0.f, 0.f};
    }
    static __device__ __forceinline__ acc_t run(const v8i &a, const v8i &b, acc_t c, int sa, int sb) {
        if constexpr (I8) {
            c = __builtin_amdgcn_mfma_i32_16x16x64_i8(v4i{a[0], a[1], a[2], a[3]}, v4i{b[0], b[1], b[2], b[3]}, c, 0, 0, 0);
            return __builtin_amdgcn_mfma_i32_16x16x64_i8(v4i{a[4], a[5], a[6], a[7]}, v4i{b[4], b[5], b[6], b[7]}, c, 0, 0, 0);
        } else {
            return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0, sa, 0, sb);
        }
    }
};

// (acc + bias) rounded to the output dtype, then -- converted per-tensor graphs, quantize_pt2e.py:323-446: the
// dequantize(s_x * s_w) node behind the GEMM -- multiplied by the dequantize factor and rounded again.
// out_bits is the one definition of that chain: the fp32 image (out_f32) or the bf16 bits of the element; emit_out stores it.
__device__ __forceinline__ uint32_t out_bits(const MxGemmArgs &a, float accv, float bv, float sv) {
    float v = accv + bv;
    if (a.out_f32) {
        if (a.out_fold_f32) v = qt_u2f(qt_fold_img(qt_f2u(v)));
        if (a.out_scale) v = v * sv;
        return qt_f2u(v);
    }
    uint16_t b = qt_f2bf(v);
    if (a.out_scale) b = qt_f2bf(qt_bf2f(b) * sv);
    return b;
}
__device__ __forceinline__ void emit_out(const MxGemmArgs &a, float accv, float bv, float sv, long idx) {
    const uint32_t b = out_bits(a, accv, bv, sv);
    if (a.out_f32) ((uint32_t *)a.C)[idx] = b;
    else ((uint16_t *)a.C)[idx] = (uint16_t)b;
}
__device__ __forceinline__ float out_scale_of(const MxGemmArgs &a, int col) {
    if (!a.out_scale) return 1.0f;
    const long i = a.out_scale_per_col ? col : 0;
    return a.out_f32 ? ((const float *)a.out_scale)[i] : qt_bf2f(((const uint16_t *)a.out_scale)[i]);
}
__device__ __forceinline__ float bias_of(const MxGemmArgs &a, int col) {
    if (!a.bias) return 0.f;
    return a.out_f32 ? ((const float *)a.bias)[col] : qt_bf2f(((const uint16_t *)a.bias)[col]);
}

// ---- codes out (qt_q8_*_codes): the epilogue writes the NEXT convolution's int8 NHWC codes instead of the value tensor -------------
// Replaces, between two conv2d_q nodes of a converted per-tensor int8 graph (quantize_pt2e.py:323-446),
//     y = dequantize(conv)  ->  aten.relu / aten.hardtanh / aten.clamp(y)  ->  quantize(., s_next, qmap_next) narrowed to int8
// i.e. the value tensor written, read and written by the activation, and read again by qt_quantize_codes_nhwc_*.  An element's
// tail: b = out_bits(...) as the value kernels compute it; v = its value in the model dtype; the clamp (NaN stays NaN, as torch's
// clamp leaves it; the result is a value of the model dtype, or a bound rounded to it); code_of(qdq_value(v)) with exactly the
// arguments qt_quantize_codes_nhwc_* builds (mode 0, no zero point, the 65 536-entry map read from global memory): qt_qdq.h.
// The tail is a kernel parameter of the CODES instantiations only: the other instantiations take NoTail, which has no field.
struct CodesTail {
    const uint16_t *qmap;        // the consumer's value map
    const void *scale;           // the consumer's activation scale, one element in the model dtype
    int act;                     // 1: clamp to [lo, hi] in front of the quantize (relu: lo = 0, hi = +inf)
    float lo, hi;
};
struct NoTail {};
template <bool CODES>
using tail_t = std::conditional_t<CODES, CodesTail, NoTail>;

__device__ __forceinline__ float next_scale_of(const MxGemmArgs &a, const CodesTail &ct) {
    return a.out_f32 ? *(const float *)ct.scale : qt_bf2f(*(const uint16_t *)ct.scale);
}
__device__ __forceinline__ uint32_t out_code(const MxGemmArgs &a, const CodesTail &ct, float ns, float accv, float bv, float sv) {
    const uint32_t b = out_bits(a, accv, bv, sv);
    float v = a.out_f32 ? qt_u2f(b) : qt_u2f(b << 16);
    if (ct.act) v = (v != v) ? v : fminf(fmaxf(v, ct.lo), ct.hi);
    const QdqArgs q{nullptr, ct.qmap, {QT_FMT_LUT, 0, 0, 0.f, 0.f}, 1, 0};
    if (a.out_f32) return code_of(qdq_value<kIoF32>(v, q, ns, 0.0f, false));
    return code_of(qdq_value<kIoBf16>(bf16_round(v), q, ns, 0.0f, false));
}

// The CODES epilogue of the two MFMA kernels.  A lane holds column l & 15 of rows 4 g + e of each 16 x 16 block: its bytes go into
// the workgroup's 128 x 128 byte tile in LDS -- the operand tiles' space, free behind the barrier that follows the last compute --
// and every thread then writes four whole 16-byte runs of a code row; rows >= M and runs >= N (N % 16 == 0) are skipped, so no
// byte outside y is written and no 1-byte store reaches memory.  The row pitch of 144 bytes (36 words) puts the two rows that a
// 32-lane half of ds_write_b8 touches (4 g + e for two g: 144 words apart) on banks 0-3 and 16-19.
constexpr int kCodePitch = kBN + 16;
template <typename ACC>
__device__ __forceinline__ void emit_codes_tile(const MxGemmArgs &a, const CodesTail &ct, uint8_t *lds, const ACC (&acc)[4][4], int m0,
                                                int n0, long cbase) {
    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int r = l & 15, g = l >> 4;
    const int wm = w >> 1, wn = w & 1;
    const float ns = next_scale_of(a, ct);
    __syncthreads();                                      // every wave has read its last fragments
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int lc = wn * 64 + j * 16 + r, col = n0 + lc;
        if (col >= a.N) continue;
        const float bv = bias_of(a, col), sv = out_scale_of(a, col);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int lr = wm * 64 + i * 16 + 4 * g + e;
                if (m0 + lr >= a.M) continue;
                lds[lr * kCodePitch + lc] = (uint8_t)out_code(a, ct, ns, (float)acc[i][j][e], bv, sv);
            }
        }
    }
    __syncthreads();
    int8_t *y = (int8_t *)a.C + cbase;
#pragma unroll
    for (int k = 0; k < kBM * (kBN / 16) / 256; ++k) {
        const int q = t + 256 * k, lr = q / (kBN / 16), run = q % (kBN / 16);
        if (m0 + lr >= a.M || n0 + run * 16 >= a.N) continue;
        *(uint4 *)(y + (long)(m0 + lr) * a.N + n0 + run * 16) = *(const uint4 *)(lds + lr * kCodePitch + run * 16);
    }
}

// LDS image of a 128-row operand tile.  8- and 4-bit tiles are unpadded with the 16-byte chunk index XOR-swizzled by
// the row so that the four 16-lane groups of ds_read_b128 ({0-3,12-15,20-27}, ... : sixteen different rows, half of
// them one chunk further along k) each touch sixteen different 16-byte slots of the 256-byte bank row; 6-bit tiles
// (96-byte rows, read with three ds_read_b64) are stored in groups of 8 rows (768 bytes) followed by 16 bytes of
// padding: a fragment's rows r and r + 8 then sit 2 eight-byte slots apart modulo the 32-slot bank row, which makes the
// two 32-lane halves of ds_read_b64 conflict-free (unpadded 96-byte rows collide pairwise: 12 r mod 32 has period 8),
// and one 48-lane LDS-DMA instruction fills exactly one group.
template <int F>
struct Tile {
    static constexpr int kRow = tile_row_bytes(F);                  // bytes of one row of a 128-deep tile
    static constexpr bool kSix = (F == 2 || F == 3);
    static constexpr int kGroup = 8 * kRow + 16;                    // 6-bit tiles: 8 rows + pad
    static constexpr int kChunks = kRow / 16;
    static constexpr int kBytes = kSix ? 16 * kGroup : 128 * kRow;
    static __device__ __forceinline__ int row_off(int row) {
        if constexpr (kSix) return (row >> 3) * kGroup + (row & 7) * kRow;
        else return row * kRow;
    }
    static __device__ __forceinline__ int chunk_off(int row, int chunk) {
        if constexpr (F < 2) return row * kRow + ((chunk ^ ((row >> 1) & 7)) << 4);
        else if constexpr (F < 4) return row_off(row) + (chunk << 4);
        else return row * kRow + ((chunk ^ ((0x78 >> (((row >> 2) & 3) * 2)) & 3)) << 4);     // f = [0,2,3,1], see below
    }
};
// fp4 swizzle: rows r and r' of one lane group with r & 3 == r' & 3 collide when f(r >> 2) ^ f(r' >> 2) == 1 for a
// row pair that sits on different k chunks; those pairs are (0|3, 1|2), so f must pair 0 with 3 and 1 with 2:
// f = [0, 2, 3, 1] (packed two bits each, low first, in 0x78).

template <int F>
__device__ __forceinline__ v8i read_frag(const uint8_t *tile, int row, int g) {
    v8i f = {0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (F < 2) {
        const uint4 lo = *(const uint4 *)(tile + Tile<F>::chunk_off(row, g));
        const uint4 hi = *(const uint4 *)(tile + Tile<F>::chunk_off(row, 4 + g));
        f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
    } else if constexpr (F < 4) {
        const uint8_t *p = tile + Tile<F>::row_off(row) + 24 * g;
        const uint2 a = *(const uint2 *)(p), b = *(const uint2 *)(p + 8), c = *(const uint2 *)(p + 16);
        f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y;
    } else {
        const uint4 lo = *(const uint4 *)(tile + Tile<F>::chunk_off(row, g));
        f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w;
    }
    return f;
}

// ---- workgroup id -> output tile ----------------------------------------------------------------------------------------------
// Workgroup ids go round-robin over the 8 XCDs; give each XCD a contiguous run of work items:
// XCD x owns [x*per + min(x, rem), ...).
__device__ __forceinline__ int xcd_run_item(int nitems, int lin) {
    const int per = nitems / 8, rem = nitems % 8, x = lin % 8, q = lin / 8;
    return x * per + (x < rem ? x : rem) + q;
}
// ... and walk the tiles in groups of GROUP M-tiles per N-tile column so that a run re-uses its A and B panels out of that XCD's
// L2.  nsplit > 1 (split of K): the work item is tile * nsplit + split through the same remap, so that the splits of a tile land on
// one XCD, next to each other.
struct TileAt {
    int m0, n0;                  // first row and column of the tile
    int id, split;               // the remapped tile id, and which of its nsplit work items this workgroup is
};
template <int TM, int TN, int GROUP>
__device__ __forceinline__ TileAt tile_at(int ntiles, int tiles_m, int tiles_n, int lin, int nsplit = 1) {
    const int item = xcd_run_item(ntiles * nsplit, lin);
    const int split = item % nsplit, id = item / nsplit;
    const int width = GROUP * tiles_n, grp = id / width, first_m = grp * GROUP;
    const int gsize = min(tiles_m - first_m, GROUP);
    return {(first_m + (id % width) % gsize) * TM, ((id % width) / gsize) * TN, id, split};
}

// ---- the dense register-staged side of an operand: rows [row0, row0 + 128) of a [rows][row_bytes] code matrix ---------------------
// Per-thread staging geometry (fixed over the k loop); rows beyond `rows` re-read the last row (never stored to C).  load(kt)
// brings the thread's 16-byte chunks of k tile kt into registers, store() puts them into the LDS image of the tile.
__device__ __forceinline__ uint4 chunk_or_zero(bool live, uint4 v) {
    // branch-free so that the k loop stays one basic block (the scheduling fences of the k loops only act inside one)
    v.x = live ? v.x : 0u; v.y = live ? v.y : 0u; v.z = live ? v.z : 0u; v.w = live ? v.w : 0u;
    return v;
}
template <int F>
struct DenseSide {
    using T = Tile<F>;
    static constexpr int kN = 128 * T::kChunks / 256;                // chunks per thread
    const uint8_t *g[kN];
    int l[kN], c[kN];
    long row_bytes;
    uint4 r[kN];
    __device__ __forceinline__ void init(const uint8_t *base, int row0, int rows, long row_bytes_) {
        row_bytes = row_bytes_;
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            const int ch = threadIdx.x + 256 * i, row = ch / T::kChunks, cc = ch % T::kChunks;
            g[i] = base + (long)min(row0 + row, rows - 1) * row_bytes + cc * 16;
            l[i] = T::chunk_off(row, cc);
            c[i] = cc * 16;
        }
    }
    __device__ __forceinline__ void load(int kt) {
        // the k tail (K % 128 != 0) re-reads chunk 0 of the row and is zeroed when it is stored
#pragma unroll
        for (int i = 0; i < kN; ++i) {
            const long off = (long)kt * T::kRow + c[i];
            r[i] = *(const uint4 *)(g[i] + (off < row_bytes ? (long)kt * T::kRow : -(long)c[i]));
        }
    }
    __device__ __forceinline__ void store(uint8_t *lds_tile, int kt) const {
#pragma unroll
        for (int i = 0; i < kN; ++i) *(uint4 *)(lds_tile + l[i]) = chunk_or_zero((long)kt * T::kRow + c[i] < row_bytes, r[i]);
    }
};

// ---- one staged k tile of the 4-wave 128 x 128 kernels: a wave's 64 x 64 quarter, 4 x 4 fragments -------------------------------
template <int FA, int FB, bool I8>
__device__ __forceinline__ void mma_tile(const uint8_t *tile_a, const uint8_t *tile_b, const int (&sa)[4], const int (&sb)[4],
                                         typename Mma<FA, FB, I8>::acc_t (&acc)[4][4]) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = l & 15, g = l >> 4;
    const int wm = w >> 1, wn = w & 1;
    v8i fa[4], fb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = read_frag<FA>(tile_a, wm * 64 + i * 16 + r, g);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = read_frag<FB>(tile_b, wn * 64 + j * 16 + r, g);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = Mma<FA, FB, I8>::run(fa[i], fb[j], acc[i][j], sa[i], sb[j]);
}

// ---- the value epilogue: D col = l & 15, row = 4 g + e -----------------------------------------------------------------------------
// A wave's NI x 4 fragments from row `row0` and column `col0` on, for lane (r, g); rows >= M and columns >= N are skipped.
// SCALED = false: the kernel has no dequantize factor -- its launchers refuse one (launch_conv, launch_mxi) -- so none is loaded
// and out_bits' second rounding is compiled out.
// The arguments come by value: through a reference the compiler would re-read the flags of `a` behind every store to C.
template <bool SCALED, int NI, typename ACC>
__device__ __forceinline__ void emit_tile(MxGemmArgs a, const ACC (&acc)[NI][4], int row0, int col0, long cbase, int r, int g) {
    if constexpr (!SCALED) a.out_scale = nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + j * 16 + r;
        if (col >= a.N) continue;
        const float bv = bias_of(a, col);
        float sv = 1.0f;
        if constexpr (SCALED) sv = out_scale_of(a, col);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = row0 + i * 16 + 4 * g + e;
                if (row >= a.M) continue;
                emit_out(a, (float)acc[i][j][e], bv, sv, cbase + (long)row * a.N + col);
            }
        }
    }
}

// The element-format pairs with a kernel, for the 256 x 256, the LDS-DMA and the plain 128 x 128 kernels and conv2d_mx alike.
using MxPairs = qt_pairs<qt_pair<0, 0>, qt_pair<0, 1>, qt_pair<1, 0>, qt_pair<1, 1>, qt_pair<2, 2>, qt_pair<3, 3>, qt_pair<4, 4>, qt_pair<0, 4>,
                         qt_pair<2, 4>, qt_pair<3, 4>>;

// What a *_codes entry point checks on top of its sibling: whole 16-byte runs of codes, the consumer's map and scale, the clamp.
inline int codes_tail_check(const CodesTail &ct, int cout, const void *y, int y_is_f32) {
    if (cout % 16 != 0 || !ct.qmap || !ct.scale || (ct.act != 0 && ct.act != 1)) return QT_ERR_BAD_ARG;
    if (ct.act == 1 && !(ct.lo <= ct.hi)) return QT_ERR_BAD_ARG;                               // false for a NaN bound too
    if (((uintptr_t)ct.qmap & 1u) || ((uintptr_t)ct.scale & (y_is_f32 ? 3u : 1u)) || ((uintptr_t)y & 15u)) return QT_ERR_UNALIGNED;
    return QT_OK;
}

}  // namespace
