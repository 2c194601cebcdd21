// qt_gemm_ring.h -- what the bf16 matrix-core kernels with k-contiguous operands share: the LDS ring of k tiles filled by LDS-DMA, the
// swizzled [rows][64 k] image, its fragment read, the counted wait + barrier, the drain of the ring and the epilogue of an output tile.
// Operands stored with the contraction index as the ROW index are staged as [64 k][columns] images and read through ds_read_b64_tr_b16
// (s_tr / off_tr / ld_frag_tr).
// Used by qt_train_gemm.hip (the Linear products of a training step), qt_conv.hip (implicit-GEMM Conv2d) and qt_conv_backward.hip (its
// input and weight gradients): a convolution differs from the GEMM only in WHERE a lane's 16 bytes of the gathered image come from.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_device.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int kBK = 64;                 // k tile
constexpr int kThreads = 512;          // 8 waves: 4 (rows) x 2 (columns); two per SIMD, so one wave's LDS latencies hide under the other's matrix instructions

// [rows][64 k] image, 128-byte rows: byte offset of 16-byte chunk `ch` (0..7) of row `row`
__device__ __forceinline__ int off_rows(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }

__device__ __forceinline__ bf16x8 ld_frag_rows(const unsigned char *img, int row, int ch) {
    return *(const bf16x8 *)(img + off_rows(row, ch));
}

// [64 k][C columns] image read by ds_read_b64_tr_b16.  RB = 2 C bytes per row (128 or 256).  A 32-lane half reads rows r0 + q and r0 + 8 + q
// (q = 0..3), 32 bytes of the same column group each: eight 32-byte pieces that must fall on eight different bank groups (64 banks x 4 B =
// eight groups of 32 B).  Row r starts at bank group (r RB / 32) mod 8 -- 0 for RB = 256, 0 or 4 for RB = 128 -- so the column group index
// is XORed with a value that is distinct over {q, 8 + q} (RB = 256) resp. over the rows of equal parity among them (RB = 128).
template <int RB>
__device__ __forceinline__ int s_tr(int row) {
    static_assert(RB == 128 || RB == 256, "row lengths of 64 and 128 columns (192: 384-byte rows start at bank group 4 r mod 8 like 128-byte ones and take their formula -- built, measured, not used)");
    if constexpr (RB == 256) return (row & 3) | (((row >> 3) & 1) << 2);
    else return ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
}
template <int RB>
__device__ __forceinline__ int off_tr(int row, int ch) {       // 16-byte chunk `ch` of k row `row`
    return row * RB + ((((ch >> 1) ^ s_tr<RB>(row))) << 5) + ((ch & 1) << 4);
}

// the fragment of 16 columns c0 .. c0 + 15 (c0 a multiple of 16) for k = k0 .. k0 + 31 of a transposed image: lane l receives column
// c0 + l % 16, k = k0 + 8 (l / 16) .. + 7
template <int RB>
__device__ __forceinline__ bf16x8 ld_frag_tr(const unsigned char *img, int c0, int k0, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int r_lo = k0 + 8 * g + q, r_hi = r_lo + 4;
    const int cp = c0 >> 4;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + r_lo * RB + ((cp ^ s_tr<RB>(r_lo)) << 5) + p * 8));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(img + r_hi * RB + ((cp ^ s_tr<RB>(r_hi)) << 5) + p * 8));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// one LDS-DMA piece: dma16 (qt_device.h), its waits counted by hand below
template <int N>
__device__ __forceinline__ void wait_and_barrier() {       // at most N of this wave's DMA pieces still in flight; LDS reads drained
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// The LDS ring: S - 1 k tiles in flight per workgroup.  Small tiles leave room for two workgroups per CU (four waves per SIMD); a ring
// over the whole CU's LDS for a single workgroup measured SLOWER on every shape (profiles/r06_train_gemm.txt): what these launches lack
// is waves to overlap, not bytes in flight.
template <int BM, int BN>
struct Ring {
    static constexpr int kStage = (BM + BN) * kBK * 2;                  // 16 / 24 / 32 KiB
    // (128 x 192: 3 x 40 KiB; a fourth stage -- the whole LDS of a CU -- changes nothing: with 24 multiplications and 16 fragment reads per
    // wave and k tile that shape is paced by the LDS reads, 0.76 us per k tile, not by the operands in flight)
    static constexpr int kStages = (BM + BN) <= 128 ? 4 : ((BM + BN) <= 192 ? 3 : ((BM + BN) <= 256 ? 4 : 3));
    static constexpr int kBytes = kStage * kStages;
};

// the last S - 1 k tiles: nothing left to request, the queue drains (D k tiles still in flight behind the one being multiplied)
template <int D, int PIECES, class F>
__device__ __forceinline__ void drain(int &kt, F &&compute) {
    wait_and_barrier<D * PIECES>();
    compute(kt++);
    if constexpr (D > 0) drain<D - 1, PIECES>(kt, compute);
}

// Workgroups go to the eight XCDs round robin (workgroup b to XCD b % 8), each with its own L2.  Where the row-tile count is a multiple
// of 8 the walk "row tiles of one column tile first" already gives an XCD two or three row tiles for ALL column tiles (it fetches an
// eighth of A and shares every B tile between its workgroups).  Where it is not (768 / 64 = 12 row tiles: the small weight gradients) an
// XCD's tiles are scattered over the whole product and every L2 fetches both operands whole; there the tiles are dealt out so that XCD x
// takes a contiguous run of the walk -- one and a half column tiles with all their row tiles.
__device__ __forceinline__ int xcd_run(int b, int total) {
    const int x = b & 7, j = b >> 3, q = total >> 3, r = total & 7;
    return x * q + (x < r ? x : r) + j;
}

// ---- epilogue of a BM x BN tile held by 4 x 2 waves (the matrix instruction's operands swapped: a lane owns four consecutive output
// COLUMNS of one row, an 8-byte store): lane (r, g) = (lane & 15, lane >> 4) of tile (i, j) holds C[row0 + r][col0 + 4 g .. + 3].  Bias in fp32, one rounding.
template <int BM, int BN>
__device__ __forceinline__ void store_tile(const f32x4 (&acc)[BM / 64][BN / 32], uint16_t *c, long ldc, const uint16_t *bias, int m0, int n0, int M,
                                           int N, int wr, int wc, int r, int g) {
    constexpr int WM = BM / 64, WN = BN / 32;
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int col = n0 + wc * (BN / 2) + j * 16 + 4 * g;
        if (col >= N) continue;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
            const uint2 b = *(const uint2 *)(bias + col);
            bv[0] = qt_u2f(b.x << 16); bv[1] = qt_u2f(b.x & 0xFFFF0000u); bv[2] = qt_u2f(b.y << 16); bv[3] = qt_u2f(b.y & 0xFFFF0000u);
        }
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            const int row = m0 + wr * (BM / 4) + i * 16 + r;
            if (row < M)
                *(uint2 *)(c + (long)row * ldc + col) = uint2{pack_bf16x2(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1]),
                                                             pack_bf16x2(acc[i][j][2] + bv[2], acc[i][j][3] + bv[3])};
        }
    }
}

}  // namespace
