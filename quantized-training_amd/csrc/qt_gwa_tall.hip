// qt_gwa_tall.hip -- the Linear over packed group-wise affine weights for MANY rows (M > 32: a prefill, a batch, an evaluation window).
//
//   qt_linear_gwa_tall_bf16    y[M, N] = rd(bias + sum_k x[m, k] Wd[n, k]),  Wd = rd(rd(q - z) s)  (gwa_dequant, qt_gwa.h)
//   qt_linear_gwa_tall_plan    the row tile, the split of K and the workspace of a shape (host only)
//
// It reads the packed layout of qt_gwa_gemm.hip as it is.  That file's kernel converts the whole weight once per 64 rows; here a
// workgroup converts a k tile of 128 columns ONCE for BM = 128 or 256 rows, into LDS, and the dequantized weight never reaches memory.
//
// Work decomposition.  A workgroup of 8 waves (4 row x 2 column, qt_gemm_ring.h) owns a BM x 128 output tile; a wave owns
// (BM / 4) x 64 of it as 16 x 16 tiles on v_mfma_f32_16x16x32_bf16 (operands swapped: a lane ends up with four consecutive columns
// of one row).  K runs in k tiles of 64 through a ring of S stages (4 at BM = 128, 3 at BM = 256: 128 / 144 KiB); a stage holds
//     the x image  [BM rows][64 k]       filled by LDS-DMA (dma16), S - 1 k tiles in flight, rows >= M clamped for reading,
//     the W image  [128 columns][64 k]   written by the waves themselves,
// both in the swizzle of off_rows, both read with ld_frag_rows.
// The W image.  The 8 column groups of the tile are dealt to the 8 waves.  A packed piece is what one wave loads with 16 bytes per
// lane: its group x one super step (128 k at 4 bits = two k tiles, 64 k at 8 bits = one).  Lane 16 g + r holds column r,
// k = 32 j + 8 g + e: its k step j is 16-byte chunk 4 (j & 1) + g of row 16 wave + r in k tile j >> 1 of the super step.  Per
// super step a lane loads its piece and its column's scale and zero point -- once per block, or once where a block spans the super
// step (NB = blocks per super step, a template argument: the number of loads in flight is counted by hand) --, converts with
// gwa_dequant and stores J chunks.  The sixteen lanes of one g write rows 16 wave + r, r = 0 .. 15, at one chunk index c: 16-byte
// bank unit (8 (r & 1) + (c ^ (r >> 1))) mod 16 -- sixteen different units, the pattern ld_frag_rows reads with.
// Step u of the k loop:  counted wait + barrier (x tile u has landed, every wave's chunks of W tile u are written, every wave is
// done with step u - 1)  ->  where the super step that starts at tile u + 1 is due: request its piece, scales and zero points  ->
// request x tile u + S - 1  ->  multiply tile u  ->  where due: wait for the piece (the x requests behind it stay in flight),
// convert, store into the stages of tiles u + 1 (and u + 2).  Those stages are free: tile u + 2 - S <= u - 1 was multiplied before
// this step's barrier (S >= KT + 1).
// Edges.  K % 32 == 0 only: chunks of either image at k >= K are ZERO chunks (packed codes there are code 0, which does not
// dequantize to zero; the x chunks there are not loaded, their DMA reads a zero row).  Column groups past the packed operand are
// clamped for reading; rows >= M and columns >= N are never stored.
// Split of K.  `ksplit` workgroups share a tile over contiguous ranges of super steps; each leaves its fp32 partial tile in the
// caller's workspace (write-through), and the one that draws the tile's last ticket adds the partial sums IN SPLIT ORDER, its own
// included, resets the ticket and runs the epilogue (the hand-over of qt_splitk.h).  Nobody waits; the bits do not depend
// on who arrived last.  fp32 accumulation in k order, bias added in fp32, one rounding to bf16; no atomics on floats, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_dispatch.h"
#include "qt_gemm_ring.h"
#include "qt_gwa.h"
#include "qt_splitk.h"

namespace {

#pragma clang fp contract(off)

__device__ __attribute__((aligned(128))) const uint32_t kZeroRow[32] = {0};      // what x chunks at k >= K and past a split's range read

constexpr int kBN = 128;                                  // columns of a tile: 8 groups of 16, one per wave
constexpr int kMaxSplit = 8;

template <int BM>
struct TallRing {
    static constexpr int kStages = BM == 128 ? 4 : 3;
    static constexpr int kXImg = BM * kBK * 2;
    static constexpr int kStage = kXImg + kBN * kBK * 2;  // 32 / 48 KiB
    static constexpr int kBytes = kStage * kStages;
};

struct Args {
    const uint16_t *x;        // [M][K] bf16
    const u32x4 *packed;      // [n16][nss][64] pieces
    const uint16_t *scale;    // [N][K / bs] bf16
    const uint16_t *zp;       // [N][K / bs] bf16
    const uint16_t *bias;     // [N] bf16 or NULL
    uint16_t *y;              // [M][N] bf16
    f32x4 *ws;                // ksplit > 1: the partial sums (splitk_slab)
    unsigned int *tickets;    // ksplit > 1: [tile] arrival counters, zero between launches
    int M, N, K;
    int nkb, bs_shift;        // K / bs, log2 bs
    int nss, n16, tiles_m, ksplit;
    float qmin;
};

// Loads whose completion is counted by hand next to the LDS-DMA requests (a load the compiler knows of is waited for with
// vmcnt(0), which also waits for every DMA piece in flight).  The value is used only behind wait_loads.
__device__ __forceinline__ u32x4 request16(const void *p) {
    u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
__device__ __forceinline__ uint32_t request_u16(const void *p) {
    uint32_t v;
    asm volatile("global_load_ushort %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
template <int YOUNGER, int NB>
__device__ __forceinline__ void wait_loads(u32x4 &pc, uint32_t (&sr)[NB], uint32_t (&zr)[NB]) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(pc) : "n"(YOUNGER) : "memory");
#pragma unroll
    for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(sr[b]), "+v"(zr[b]));
}

// the eight bf16 values of k step j of a lane's piece, as one 16-byte chunk
template <int BITS>
__device__ __forceinline__ u32x4 chunk_of(const u32x4 &p, int j, float qmin, float z, float s) {
    float q[8];
    piece_codes<BITS>(p, j, qmin, q);
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = gwa_dequant<kIoBf16>(q[e], z, s);
    return u32x4{pack_bf16x2(q[0], q[1]), pack_bf16x2(q[2], q[3]), pack_bf16x2(q[4], q[5]), pack_bf16x2(q[6], q[7])};
}

template <int BITS, int BM, int NB>
__global__ __launch_bounds__(kThreads) void linear_gwa_tall_kernel(const Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    constexpr int J = Geo<BITS>::kJ, SK = Geo<BITS>::kSK, KT = SK / kBK;     // KT: k tiles per super step
    constexpr int S = TallRing<BM>::kStages, kXImg = TallRing<BM>::kXImg, kStage = TallRing<BM>::kStage;
    constexpr int kAV = BM / 64;                                          // DMA pieces (1 KiB) per wave and k tile
    constexpr int WM = BM / 64, WN = kBN / 32;
    static_assert(S >= KT + 1, "a super step is converted into stages that are free");
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), wr = wave >> 1, wc = wave & 1;
    const int r = lane & 15, g = lane >> 4;
    const int split = (int)blockIdx.x % a.ksplit, tile = (int)blockIdx.x / a.ksplit;
    const int tn = tile / a.tiles_m, tm = tile % a.tiles_m;               // the row tiles of a column tile are neighbours
    const int m0 = tm * BM, n0 = tn * kBN;
    // this split's super steps, k range and k tiles
    const int ss0 = (int)((long)split * a.nss / a.ksplit), ss1 = (int)((long)(split + 1) * a.nss / a.ksplit);
    const int kbeg = ss0 * SK, kend = min(a.K, ss1 * SK);
    const int nt = ss1 > ss0 ? (kend - kbeg + kBK - 1) / kBK : 0;

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nt > 0) {
        // ---- x: DMA sources of the split's first k tile; piece v of this wave is image piece v * 8 + wave (8 rows of 128 bytes)
        const unsigned char *const zero = (const unsigned char *)kZeroRow + (lane & 7) * 16;
        const unsigned char *sx[kAV];
        uint32_t dx[kAV];
        int kx[kAV];                                                      // k of the lane's chunk in the tile about to be requested
#pragma unroll
        for (int v = 0; v < kAV; ++v) {
            const int piece = v * 8 + wave, row = piece * 8 + (lane >> 3), pos = lane & 7, ch = pos ^ ((row >> 1) & 7);
            dx[v] = piece * 1024;
            kx[v] = kbeg + ch * 8;
            sx[v] = (const unsigned char *)(a.x + (long)min(m0 + row, a.M - 1) * a.K + kx[v]);
        }
        const uint32_t l0 = lds_addr(lds);
        int rq_stage = 0;
        auto request = [&]() __attribute__((always_inline)) {             // the next k tile -> the next stage; past the range: zeros
            const uint32_t st = l0 + rq_stage * kStage;
#pragma unroll
            for (int v = 0; v < kAV; ++v) {
                dma16(kx[v] < kend ? sx[v] : zero, st + dx[v]);
                sx[v] += kBK * 2;
                kx[v] += kBK;
            }
            rq_stage = rq_stage + 1 == S ? 0 : rq_stage + 1;
        };

        // ---- W: this wave's column group, this lane's column (clamped for reading), piece, scales and zero points of a super step
        const int ng = min(n0 / 16 + wave, a.n16 - 1);
        const long nrow = min(ng * 16 + r, a.N - 1);
        const uint16_t *const srow = a.scale + nrow * a.nkb, *const zrow = a.zp + nrow * a.nkb;
        const u32x4 *const wp = a.packed + (long)ng * a.nss * 64 + lane;
        u32x4 pc;
        uint32_t sr[NB], zr[NB];
        auto request_w = [&](int ss) __attribute__((always_inline)) {     // 1 + 2 NB loads
            pc = request16(wp + (long)ss * 64);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int kb = min(((ss * SK) >> a.bs_shift) + (NB > 1 ? b : 0), a.nkb - 1);      // (blocks beyond K: clamped, unused)
                sr[b] = request_u16(srow + kb);
                zr[b] = request_u16(zrow + kb);
            }
        };
        const int wrow = wave * 16 + r;
        auto convert = [&](int ss, int stage) __attribute__((always_inline)) {      // super step ss -> the W images of `stage` (and the next)
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int b = j * NB / J;
                u32x4 c = chunk_of<BITS>(pc, j, a.qmin, qt_u2f(zr[b] << 16), qt_u2f(sr[b] << 16));
                if (ss * SK + j * 32 >= a.K) c = u32x4{0u, 0u, 0u, 0u};   // K % 32 == 0: a k step is inside K or outside
                int st = stage + (j >> 1);
                st = st >= S ? st - S : st;
                *(u32x4 *)(lds + st * kStage + kXImg + off_rows(wrow, 4 * (j & 1) + g)) = c;
            }
        };

        int cp_stage = 0;
        auto compute = [&]() __attribute__((always_inline)) {
            const unsigned char *ia = lds + cp_stage * kStage, *ib = ia + kXImg;
#pragma unroll
            for (int ks = 0; ks < kBK / 32; ++ks) {
                bf16x8 fa[WM], fb[WN];
#pragma unroll
                for (int i = 0; i < WM; ++i) fa[i] = ld_frag_rows(ia, wr * (BM / 4) + i * 16 + r, ks * 4 + g);
#pragma unroll
                for (int j = 0; j < WN; ++j) fb[j] = ld_frag_rows(ib, wc * (kBN / 2) + j * 16 + r, ks * 4 + g);
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
            }
        };

        // ---- prologue: the first super step, x tiles 0 .. S - 2 (tiles past the range are zero tiles: the counts stay fixed)
        request_w(ss0);
#pragma unroll
        for (int i = 0; i < S - 1; ++i) request();
        wait_loads<(S - 1) * kAV, NB>(pc, sr, zr);
        convert(ss0, 0);
        // ---- k loop.  The wait leaves the (S - 2) kAV youngest requests in flight: x tiles u + 1 .. u + S - 2 (a super step's loads
        // lie in front of the x requests of their step and have been waited for)
        for (int u = 0; u < nt; ++u) {
            wait_and_barrier<(S - 2) * kAV>();
            const bool due = (u + 1) % KT == 0 && u + 1 < nt;             // (uniform) the super step whose first tile is u + 1
            const int ss = ss0 + (u + 1) / KT;
            if (due) request_w(ss);
            request();
            compute();
            cp_stage = cp_stage + 1 == S ? 0 : cp_stage + 1;
            if (due) {
                wait_loads<kAV, NB>(pc, sr, zr);
                convert(ss, cp_stage);
            }
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");         // the zero tiles requested past the range
    }

    if (a.ksplit > 1) {                                                   // the hand-over of qt_splitk.h
        f32x4 *const mine = splitk_slab<8, WM * WN>(a.ws, tile, a.ksplit, split);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) store16_sc1(mine + (i * WN + j) * 64, splitk_lane_off(), acc[i][j]);
        // (the ring is dead behind the draw's first barrier: the ticket travels through its first word)
        if ((int)splitk_draw(a.tickets + tile, 1u, (volatile unsigned int *)lds) != a.ksplit - 1) return;      // not the last one: done
        splitk_own(a.tickets + tile);
        splitk_sum<8>(acc, a.ws, tile, a.ksplit);                         // ALL the partial sums, its own included
    }
    store_tile<BM, kBN>(acc, a.y, (long)a.N, a.bias, m0, n0, a.M, a.N, wr, wc, r, g);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
struct TallPlan {
    int bm, ksplit, tiles_m, tiles_n;
    long tiles() const { return (long)tiles_m * tiles_n; }
    size_t ws_bytes() const { return ksplit > 1 ? (size_t)tiles() * ksplit * bm * kBN * 4 : 0; }
    size_t tickets() const { return ksplit > 1 ? (size_t)tiles() : 0; }
};

// A fixed function of the shape and the CU count.  256-row tiles where they alone give every other CU a workgroup (the conversion
// cost per weight halves again), else 128-row tiles.  K is split while the tiles leave CUs idle: tiles x split <= CUs, at least
// two super steps per split (the ring's fill and the hand-over stay small beside its work), 8 splits at the most.
TallPlan tall_plan(int M, int N, int K, int bits, int tile_m, int ksplit) {
    TallPlan p{};
    const long cus = qt_cu_count();
    const long tn = (N + kBN - 1) / kBN;
    p.bm = tile_m ? tile_m : (M > 128 && (long)((M + 255) / 256) * tn * 2 >= cus ? 256 : 128);
    p.tiles_m = (M + p.bm - 1) / p.bm;
    p.tiles_n = (int)tn;
    p.ksplit = ksplit;
    if (!ksplit) {
        const long nss = gwa_nss(K, bits);
        p.ksplit = 1;
        for (int s = 2; s <= kMaxSplit && p.tiles() * s <= cus && nss / s >= 2; s *= 2) p.ksplit = s;
    }
    return p;
}

template <int BITS, int BM, int NB>
int launch(const Args &a, long grid, hipStream_t st) {
    constexpr int kLds = TallRing<BM>::kBytes;
    static_assert(kLds <= 160 * 1024, "the ring does not fit a CU's LDS");
    if (const int rc = qt_allow_lds<linear_gwa_tall_kernel<BITS, BM, NB>>(kLds)) return rc;
    linear_gwa_tall_kernel<BITS, BM, NB><<<(unsigned)grid, kThreads, kLds, st>>>(a);
    return qt_launch_status();
}

}  // namespace

extern "C" {

int qt_linear_gwa_tall_plan(int M, int N, int K, int bits, int tile_m, int *tile_m_out, int *ksplit_out, size_t *ws_bytes, size_t *n_tickets) {
    if (M < 0 || !(tile_m == 0 || tile_m == 128 || tile_m == 256)) return QT_ERR_BAD_ARG;
    if (const int rc = gwa_shape_status(N, K, bits)) return rc;
    const TallPlan p = tall_plan(M, N, K, bits, tile_m, 0);
    if (tile_m_out) *tile_m_out = p.bm;
    if (ksplit_out) *ksplit_out = p.ksplit;
    if (ws_bytes) *ws_bytes = p.ws_bytes();
    if (n_tickets) *n_tickets = p.tickets();
    return QT_OK;
}

int qt_linear_gwa_tall_bf16(const uint16_t *x_dev, const uint8_t *packed_dev, const uint16_t *scale_dev, const uint16_t *zp_dev,
                            const uint16_t *bias_dev, uint16_t *y_dev, int M, int N, int K, int block_size, int bits, float quant_min, int tile_m,
                            int ksplit, float *ws_dev, size_t ws_bytes, uint32_t *tickets_dev, size_t n_tickets, void *stream) {
    int shift;
    const bool knobs_ok = (tile_m == 0 || tile_m == 128 || tile_m == 256) && (ksplit == 0 || ksplit == 1 || ksplit == 2 || ksplit == 4 || ksplit == 8);
    if (const int rc = linear_gwa_status(x_dev, packed_dev, scale_dev, zp_dev, bias_dev, y_dev, M, N, K, block_size, bits, knobs_ok, shift)) return rc;
    if (M == 0) return QT_OK;
    const TallPlan p = tall_plan(M, N, K, bits, tile_m, ksplit);
    if (p.ksplit > 1) {
        if (const int rc = qt_splitk_scratch_status(ws_dev, ws_bytes, p.ws_bytes(), tickets_dev, n_tickets, p.tickets())) return rc;
    }
    const long grid = p.tiles() * p.ksplit;
    if (grid > 0x7FFFFFFFL) return QT_ERR_BAD_ARG;
    Args a{};
    a.x = x_dev; a.packed = (const u32x4 *)packed_dev; a.scale = scale_dev; a.zp = zp_dev; a.bias = bias_dev; a.y = y_dev;
    a.ws = (f32x4 *)ws_dev; a.tickets = tickets_dev;
    a.M = M; a.N = N; a.K = K;
    a.nkb = K / block_size; a.bs_shift = shift;
    a.nss = (int)gwa_nss(K, bits); a.n16 = (N + 15) / 16; a.tiles_m = p.tiles_m; a.ksplit = p.ksplit;
    a.qmin = quant_min;
    hipStream_t st = (hipStream_t)stream;
    // blocks per super step: the scale and zero-point loads of a conversion (1 where a block spans the super step)
    const int sk = bits == 4 ? 128 : 64, nb = block_size >= sk ? 1 : sk / block_size;
    int rc = QT_ERR_BAD_ARG;
    qt_pick_pair(qt_pairs<qt_pair<4, 1>, qt_pair<4, 2>, qt_pair<4, 4>, qt_pair<8, 1>, qt_pair<8, 2>>{}, bits, nb, [&](auto P) {
        using T = decltype(P);
        rc = p.bm == 128 ? launch<T::a, 128, T::b>(a, grid, st) : launch<T::a, 256, T::b>(a, grid, st);
    });
    return rc;
}

}  // extern "C"
