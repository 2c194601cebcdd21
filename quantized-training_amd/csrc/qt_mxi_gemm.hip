// Block-scaled GEMM for integer and codebook operands under arbitrary block scales (qt_mxi_pack / qt_mxi_gemm).
//
// linear_mx / matmul_mx (decomposed.py:304-363) for what the scaled float instruction cannot read: intN elements, integer
// codebooks, block scales that are no powers of two.  Operand: int8 codes[rows][K] and fp32 scales[rows][K / BS].
//     C[m][n] = rd( bias[n] + sum_kb (sA[m][kb] sB[n][kb]) * (sum_{k in block kb} a[m][k] b[n][k]) )
// The inner sum is one block on the integer matrix cores, exact in int32 (|p| <= 128 * 128 * 128 < 2^24, so its conversion to
// fp32 is exact as well); t = sA * sB is one fp32 product; acc = fma(p, t, acc) with the blocks in increasing kb; bias added in
// fp32, one rounding to the output dtype (emit_out).  No atomics, no split-K: the same bits on every launch.
// The register-staged 128 x 128 x 128 kernel of qt_mx_gemm.hip (same tile image, same staging, same tail rules) with the block scales of a
// k tile staged through LDS next to the codes: s[operand][block of the tile][row of the tile] fp32, so that a lane reads the
// scales of its four accumulator rows (4 g + e) of a fragment tile with one 16-byte read.
//   BS = 128: two v_mfma_i32_16x16x64_i8 accumulate in int32 before the conversion;   BS = 64: one per block;
//   BS = 32: v_mfma_i32_16x16x32_i8, eight bytes per lane.  A dot product does not depend on which k of the 32 a lane's byte is
//   taken for as long as both operands use the same assignment (they do: both fragments are read by read_frag32) and the four
//   lane groups together hold each k of the block once: group g reads bytes [8 g, 8 g + 8) of the block.
#include "qt_mx_tile.h"

namespace {

template <int BS>
struct Mxi {
    static constexpr int kScales = kBK / BS;                              // block scales per row and k tile
    static constexpr int kScaleFloats = 2 * kScales * 128;                // one stage: both operands
    static constexpr int kLds = 4 * Tile<0>::kBytes + 2 * kScaleFloats * 4;
};

// the four 32-blocks of a 128-deep tile row, eight bytes each: f[2 blk], f[2 blk + 1]
__device__ __forceinline__ v8i read_frag32(const uint8_t *tile, int row, int g) {
    v8i f;
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        const uint2 v = *(const uint2 *)(tile + Tile<0>::chunk_off(row, 2 * blk + (g >> 1)) + 8 * (g & 1));
        f[2 * blk] = v.x;
        f[2 * blk + 1] = v.y;
    }
    return f;
}

// the exact int32 sum of block `blk` of the k tile for one 16 x 16 output tile
template <int BS>
__device__ __forceinline__ v4i mxi_block(const v8i &a, const v8i &b, int blk) {
    const v4i z = {0, 0, 0, 0};
    if constexpr (BS == 32) {
        const long la = (long)(((unsigned long)(uint32_t)a[2 * blk + 1] << 32) | (uint32_t)a[2 * blk]);
        const long lb = (long)(((unsigned long)(uint32_t)b[2 * blk + 1] << 32) | (uint32_t)b[2 * blk]);
        return __builtin_amdgcn_mfma_i32_16x16x32_i8(la, lb, z, 0, 0, 0);
    } else if constexpr (BS == 64) {
        const int o = 4 * blk;
        return __builtin_amdgcn_mfma_i32_16x16x64_i8(v4i{a[o], a[o + 1], a[o + 2], a[o + 3]}, v4i{b[o], b[o + 1], b[o + 2], b[o + 3]}, z, 0, 0, 0);
    } else {
        return Mma<0, 0, true>::run(a, b, z, 0, 0);
    }
}

template <int BS>
__global__ __launch_bounds__(256) void mxi_gemm_kernel(MxGemmArgs a) {
    using T = Tile<0>;
    constexpr int NS = Mxi<BS>::kScales;
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
    const long bz = blockIdx.y;
    const int nblk = a.K / BS;
    const int nk = (a.K + kBK - 1) / kBK;

    // staging geometry; rows beyond M / N re-read the last row (never stored to C).  Both operands are int8 rows of a.K bytes, so one
    // LDS offset, one k-tail redirect and one predicate per chunk serve the two of them (two DenseSide<0> would compute each twice:
    // 1 % of the kernel's time at 2048 x 4096 x 4096)
    constexpr int R = T::kRow, CH = T::kChunks;                   // 128 bytes, 8 chunks per tile row
    constexpr int NC = kBM * CH / 256;                            // chunks per thread and operand
    const long kb_row = a.K;                                      // bytes per code row
    const uint8_t *Ab = a.A + bz * a.bA, *Bb = a.B + bz * a.bB;
    const uint8_t *ga[NC], *gb[NC];
    int la[NC], ca[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = t + 256 * i, row = c / CH, cc = c % CH;
        ga[i] = Ab + (long)min(m0 + row, a.M - 1) * kb_row + cc * 16;
        gb[i] = Bb + (long)min(n0 + row, a.N - 1) * kb_row + cc * 16;
        la[i] = T::chunk_off(row, cc);
        ca[i] = cc * 16;
    }
    // thread (operand t >> 7, tile row t & 127) stages that row's block scales of the k tile
    const int sop = t >> 7, srow = t & 127;
    const float *ps = sop ? (const float *)(a.sB + bz * a.bsB) + (long)min(n0 + srow, a.N - 1) * nblk
                          : (const float *)(a.sA + bz * a.bsA) + (long)min(m0 + srow, a.M - 1) * nblk;

    uint4 ra[NC], rb[NC];
    float rs[NS];
    auto load_tile = [&](int kt) __attribute__((always_inline)) {
        // the k tail re-reads chunk 0 of the row / the row's last scale; both are replaced by zeros when they are stored
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const long off = (long)kt * R + ca[i];
            const long rel = off < kb_row ? (long)kt * R : -(long)ca[i];
            ra[i] = *(const uint4 *)(ga[i] + rel);
            rb[i] = *(const uint4 *)(gb[i] + rel);
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) rs[q] = ps[min(kt * NS + q, nblk - 1)];
    };
    auto store_tile = [&](int buf, int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const bool live = (long)kt * R + ca[i] < kb_row;
            *(uint4 *)(s_a(buf) + la[i]) = chunk_or_zero(live, ra[i]);
            *(uint4 *)(s_b(buf) + la[i]) = chunk_or_zero(live, rb[i]);
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) s_s(buf)[(sop * NS + q) * 128 + srow] = kt * NS + q < nblk ? rs[q] : 0.f;
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
        for (int blk = 0; blk < NS; ++blk) {                      // increasing kb
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

    // epilogue: D col = l & 15, row = 4 g + e
    emit_tile<false>(a, acc, m0 + wm * 64, n0 + wn * 64, bz * a.bC, r, g);
}

template <int BS>
int launch_mxi(const MxGemmArgs &g, dim3 grid, hipStream_t st) {
    if (g.out_scale) return QT_ERR_BAD_ARG;                 // the kernel compiles the dequantize factor out (emit_tile<false>)
    if (const int rc = qt_allow_lds<mxi_gemm_kernel<BS>>(Mxi<BS>::kLds)) return rc;
    mxi_gemm_kernel<BS><<<grid, 256, Mxi<BS>::kLds, st>>>(g);
    return qt_launch_status();
}

// (values or codebook indices, block scales) -> int8 codes + fp32 scales.  One thread per (row, 16 elements): one 16-byte store.
struct MxiPackArgs {
    const void *x, *scale, *code;    // values / indices and block scales and (nullable) codebook, all bf16 or all f32
    int8_t *codes;
    float *scales;
    long rows, K;
    long x_rs, x_ks, s_rs, s_ks;     // element strides
    long batch, x_bs, s_bs;
    int block_size, f32, n_code;
    int *bad;
};

__global__ __launch_bounds__(256) void mxi_pack_kernel(MxiPackArgs p) {
    __shared__ float s_code[256];
    for (int i = threadIdx.x; i < p.n_code; i += 256)
        s_code[i] = p.f32 ? ((const float *)p.code)[i] : qt_bf2f(((const uint16_t *)p.code)[i]);
    __syncthreads();
    const long ng = p.K / 16, nblk = p.K / p.block_size;
    const long total = p.batch * p.rows * ng;
    const bool rows_fast = p.x_rs == 1;                           // adjacent threads walk the contiguous dimension
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long b, row, grp;
        if (rows_fast) { row = i % p.rows; grp = (i / p.rows) % ng; b = i / (p.rows * ng); }
        else { grp = i % ng; row = (i / ng) % p.rows; b = i / (p.rows * ng); }
        bool bad = false;
        uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long xi = b * p.x_bs + row * p.x_rs + (grp * 16 + e) * p.x_ks;
            float v = p.f32 ? ((const float *)p.x)[xi] : qt_bf2f(((const uint16_t *)p.x)[xi]);
            if (p.n_code > 0) {                                   // code[x.to(torch.long)]: truncation toward zero
                int idx = 0;
                if (!(fabsf(v) < 1e9f)) bad = true;               // NaN, infinities, anything no codebook reaches
                else idx = (int)v;
                if (idx < 0 || idx >= p.n_code) { bad = true; idx = idx < 0 ? 0 : p.n_code - 1; }
                v = s_code[idx];
            }
            if (!(v >= -128.f && v <= 127.f) || v != truncf(v)) bad = true;
            const int c = v != v ? 0 : (int)fminf(fmaxf(v, -128.f), 127.f);      // saturates
            out[e >> 2] |= (uint32_t)(uint8_t)c << (8 * (e & 3));
        }
        *(uint4 *)(p.codes + (b * p.rows + row) * p.K + grp * 16) = uint4{out[0], out[1], out[2], out[3]};
        if ((grp * 16) % p.block_size == 0) {
            const long blk = grp * 16 / p.block_size;
            const long sidx = b * p.s_bs + row * p.s_rs + blk * p.s_ks;
            const float s = p.f32 ? ((const float *)p.scale)[sidx] : qt_bf2f(((const uint16_t *)p.scale)[sidx]);
            if (!(s > 0.f) || !(s < __builtin_inff())) bad = true;
            p.scales[(b * p.rows + row) * nblk + blk] = s;
        }
        if (bad && p.bad) atomicOr(p.bad, 1);
    }
}

}  // namespace

extern "C" {

int qt_mxi_pack(const void *x_dev, const void *scale_dev, int is_f32, const void *code_dev, int n_code, int8_t *codes_dev, float *scales_dev,
                long batch, long rows, long K, long x_batch_stride, long x_row_stride, long x_k_stride, long s_batch_stride,
                long s_row_stride, long s_k_stride, int block_size, int *bad_dev, void *stream) {
    if (!x_dev || !scale_dev || !codes_dev || !scales_dev || batch < 0 || batch > 65535 || rows < 0 || K < 0) return QT_ERR_BAD_ARG;
    if (block_size != 32 && block_size != 64 && block_size != 128) return QT_ERR_BAD_ARG;
    if (K % block_size != 0 || (code_dev ? n_code < 1 || n_code > 256 : n_code != 0)) return QT_ERR_BAD_ARG;
    const uintptr_t elem = is_f32 ? 3u : 1u;
    if (((uintptr_t)codes_dev & 15u) || ((uintptr_t)scales_dev & 3u) || (((uintptr_t)x_dev | (uintptr_t)scale_dev | (uintptr_t)code_dev) & elem) ||
        ((uintptr_t)bad_dev & 3u))
        return QT_ERR_UNALIGNED;
    if (batch * rows * K == 0) return QT_OK;
    MxiPackArgs p{x_dev, scale_dev, code_dev, codes_dev, scales_dev, rows, K, x_row_stride, x_k_stride, s_row_stride, s_k_stride,
                  batch, x_batch_stride, s_batch_stride, block_size, is_f32, n_code, bad_dev};
    const long total = batch * rows * (K / 16);
    unsigned grid = (unsigned)((total + 255) / 256);
    if (grid > 65535u * 4u) grid = 65535u * 4u;
    mxi_pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(p);
    return qt_launch_status();
}

int qt_mxi_gemm(const int8_t *a_codes, const float *a_scales, const int8_t *b_codes, const float *b_scales, int block_size, void *c_dev,
                int c_is_f32, const void *bias_dev, long batch, int M, int N, int K, long a_batch_stride_rows, long b_batch_stride_rows,
                void *stream) {
    if (!a_codes || !a_scales || !b_codes || !b_scales || !c_dev || batch < 0 || batch > 65535 || M < 0 || N < 0 || K < 1) return QT_ERR_BAD_ARG;
    if (block_size != 32 && block_size != 64 && block_size != 128) return QT_ERR_BAD_ARG;
    if (K % block_size != 0 || a_batch_stride_rows < 0 || b_batch_stride_rows < 0) return QT_ERR_BAD_ARG;
    const uintptr_t elem = c_is_f32 ? 3u : 1u;
    if ((((uintptr_t)a_codes | (uintptr_t)b_codes) & 15u) || (((uintptr_t)a_scales | (uintptr_t)b_scales) & 3u) ||
        (((uintptr_t)c_dev | (uintptr_t)bias_dev) & elem))
        return QT_ERR_UNALIGNED;
    const long tiles = (long)((N + kBN - 1) / kBN) * ((M + kBM - 1) / kBM);
    if (tiles >= (1L << 31)) return QT_ERR_BAD_ARG;
    if (batch * M * N == 0) return QT_OK;
    const long nblk = K / block_size;
    MxGemmArgs g{(const uint8_t *)a_codes, (const uint8_t *)b_codes, (const uint8_t *)a_scales, (const uint8_t *)b_scales, c_dev, bias_dev,
                 M, N, K, a_batch_stride_rows * (long)K, b_batch_stride_rows * (long)K, a_batch_stride_rows * nblk * 4, b_batch_stride_rows * nblk * 4,
                 (long)M * N, c_is_f32, nullptr, 0, 0};
    const dim3 grid((unsigned)tiles, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    if (block_size == 32) return launch_mxi<32>(g, grid, st);
    if (block_size == 64) return launch_mxi<64>(g, grid, st);
    return launch_mxi<128>(g, grid, st);
}

}  // extern "C"
