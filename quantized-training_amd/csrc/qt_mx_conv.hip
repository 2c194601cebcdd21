// Convolutions on packed codes: conv2d_mx on the block-scaled matrix instruction (qt_conv2d_mx), the int8 convolutions of converted
// per-tensor graphs on the integer one (qt_q8_conv2d* with the split of K and the codes-out chain) and their depthwise kernel
// (qt_q8_dwconv2d*).  Tile image, matrix step, dense B side, tile map and epilogues: qt_mx_tile.h.
#include "qt_mx_tile.h"

namespace {

// ---- conv2d_mx as an implicit GEMM (decomposed.py:265-301) --------------------------------------------------
// The register-staged 128 x 128 x 128 kernel of qt_mx_gemm.hip with a gathered A side.  Rows = output pixels (n, ho, wo), columns = Cout,
// K = kh kw Cin ordered (r, s, c).  The B operand is the packed [Cout][kh kw Cin] weight as it stands.  The A operand has no
// matrix in memory: x codes are NHWC with P = Cin bits / 8 bytes per pixel (a multiple of 16), so the 16-byte chunk at byte b
// of the virtual kh kw P-byte row of an output pixel is bytes [b % P, b % P + 16) of input pixel
// (ho sh - ph + r dh, wo sw - pw + s dw) with (r, s) = tap b / P -- a chunk never straddles a tap -- and the scale byte of
// 32-block kb is block kb % (Cin / 32) of tap kb / (Cin / 32).  A tap in the zero padding, a row past M and the K tail store
// zero chunks (code 0 is +0 in all five formats) and multiply them by the scale 1; their loads are redirected to byte 0 of the
// operand, so no address outside x_codes / x_e8m0 is ever formed into a load.
// A k tile starts at 32-block u_blk of tap (u_tr, u_ts): wave-uniform, moved on by additions.  A lane's chunk or scale byte
// lies at most four taps further (128 k over Cin >= 32), found by comparisons; a lane's pixel never changes over the k loop.
struct MxConvGeom {
    int H, W, kh, kw, sh, sw, ph, pw, dh, dw, Ho, Wo;
    int cpb;                      // 32-blocks per input pixel, Cin / 32
};

// position v (< 5 per) counted from the start of tap (tr0, ts0 < kw) -> offset inside its tap, and that tap
__device__ __forceinline__ void conv_tap_of(int v, int per, int ts0, int tr0, int kw, int &off, int &ts, int &tr) {
    const int q = (v >= per) + (v >= 2 * per) + (v >= 3 * per) + (v >= 4 * per);
    const int s = ts0 + q;                                            // < kw + 4 <= 5 kw
    const int wrap = (s >= kw) + (s >= 2 * kw) + (s >= 3 * kw) + (s >= 4 * kw);
    off = v - q * per;
    ts = s - wrap * kw;
    tr = tr0 + wrap;
}

// ---- split of K (qt_q8_conv2d_ws, I8 only) -----------------------------------------------------------------------------------------
// A long contraction over few output tiles (a reducing 1 x 1 layer, a small batch) leaves most of the chip idle.  S workgroups
// then share a tile: split s walks the k tiles [s nk / S, (s + 1) nk / S) (S <= nk: none is empty) and leaves its 64 int32 sums per
// thread in the caller's workspace, [tile][split][fragment 4 i + j][thread] of int4: a wave's store is one contiguous KiB.  The
// hand-over is the one of qt_conv_backward.hip / qt_linear_fqt.hip: write-through stores, drained by every wave in front of the
// workgroup barrier; one lane then draws the tile's ticket (relaxed, agent scope).  Whoever draws the last ticket owns the tile:
// it reads the other S - 1 partial sums past its L1, adds them AS INTEGERS to the sums it holds in registers (exact in any order:
// kh kw Cin < 2^17 bounds every partial and the total below 2^31, so the result is bit for bit the unsplit kernel's, whoever
// arrives last), resets the ticket and runs the unchanged epilogue with its single float(acc).  Nobody waits for anybody; tickets
// are zero between launches.  The owner is not known before the ticket is drawn, so every split stores (the owner's own 64 KiB
// are never read).  Like the tail of the CODES instantiations the split state is a kernel parameter of the SPLIT instantiations only.
struct SplitK {
    v4i *ws;                     // [tile][split][16 fragments][256 threads]
    unsigned int *tickets;       // [tile], zero between launches
    int S;
};
struct NoSplit {};
template <bool SPLIT>
using split_t = std::conditional_t<SPLIT, SplitK, NoSplit>;
constexpr long kSplitSlab = 16L * 256;        // int4 per tile and split: 64 KiB

// The compiler pads nothing inside an asm string and knows no hazard of the instruction in it.  Two are live here: the base is
// computed by scalar adds right in front (an SGPR written by the SALU needs wait states before a vector memory instruction reads it:
// s_nop 4 opens the string), and the sums are copied out of the accumulation registers into the same four VGPRs for every fragment
// (a 16-byte store reads its data over several cycles: s_nop 1 ends the string, so that the next copy cannot overwrite them).
__device__ __forceinline__ void store16_sc1(const v4i *sbase, uint32_t voff, v4i v) {
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ v4i load16_sc1(const v4i *sbase, uint32_t voff) {
    v4i v;
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 sc1" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
    return v;
}

// I8 (qt_q8_conv2d): int8 codes on both sides, int32 accumulators, no scale bytes -- every scale load below is compiled out --
// and the dequantize factor of emit_out in the epilogue.
template <int FA, int FB, bool I8 = false, bool CODES = false, bool SPLIT = false>
__global__ __launch_bounds__(256) void mx_conv_kernel(MxGemmArgs a, MxConvGeom c, tail_t<CODES> ct = {}, split_t<SPLIT> sp = {}) {
    static_assert(!SPLIT || I8, "only integer partial sums add exactly in any order");
    using M_ = Mma<FA, FB, I8>;
    using TA = Tile<FA>;
    using TB = Tile<FB>;
    constexpr int RA = TA::kRow, CA = TA::kChunks;
    constexpr int NA = kBM * CA / 256;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    auto s_a = [&](int buf) __attribute__((always_inline)) { return lds + buf * TA::kBytes; };
    auto s_b = [&](int buf) __attribute__((always_inline)) { return lds + 2 * TA::kBytes + buf * TB::kBytes; };

    const int t = threadIdx.x, l = t & 63, w = t >> 6;
    const int r = l & 15, g = l >> 4;
    const int wm = w >> 1, wn = w & 1;
    const int tiles_m = (a.M + kBM - 1) / kBM, tiles_n = (a.N + kBN - 1) / kBN;
    int nsplit = 1;
    if constexpr (SPLIT) nsplit = sp.S;
    const TileAt at = tile_at<kBM, kBN, 8>(tiles_m * tiles_n, tiles_m, tiles_n, blockIdx.x, nsplit);
    const int m0 = at.m0, n0 = at.n0, id = at.id, split = at.split;
    const long kbB = (long)a.K * elem_bits(FB) / 8;
    const int nblk = a.K / 32;
    const int nk = (a.K + kBK - 1) / kBK;
    const int pbytes = c.cpb * (RA / 4);                             // P: code bytes of one input pixel
    int kt0 = 0, kt1 = nk;                                          // this workgroup's k tiles
    if constexpr (SPLIT) {
        kt0 = (int)((long)split * nk / sp.S);
        kt1 = (int)((long)(split + 1) * nk / sp.S);
    }

    // an output pixel's input corner: the pixel index it would have (modulo 2^32: only taps inside the plane are fetched) and its
    // row / column; rows past M get a corner that no tap brings back into the plane
    auto corner = [&](int m, uint32_t &pix, int &hi0, int &wi0) __attribute__((always_inline)) {
        const bool live = m < a.M;
        const int mm = live ? m : 0;
        const int n = mm / (c.Ho * c.Wo), rem = mm - n * (c.Ho * c.Wo), ho = rem / c.Wo, wo = rem - ho * c.Wo;
        hi0 = live ? ho * c.sh - c.ph : -(1 << 28);
        wi0 = wo * c.sw - c.pw;
        pix = (uint32_t)n * (uint32_t)(c.H * c.W) + (uint32_t)hi0 * (uint32_t)c.W + (uint32_t)wi0;
    };
    uint32_t ga[NA], gs[4];          // byte offsets of the corners into x_codes (+ the chunk) / x_e8m0
    int hia[NA], wia[NA], his[4], wis[4];
    int la[NA], ca[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int ch = t + 256 * i, row = ch / CA, cc = ch % CA;
        uint32_t pix;
        corner(m0 + row, pix, hia[i], wia[i]);
        ga[i] = pix * (uint32_t)pbytes;
        la[i] = TA::chunk_off(row, cc);
        ca[i] = cc * 16;
    }
    DenseSide<FB> B;
    B.init(a.B, n0, a.N, kbB);
    const uint8_t *psb[4];
    if constexpr (!I8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t pix;
            corner(m0 + wm * 64 + i * 16 + r, pix, his[i], wis[i]);
            gs[i] = pix * (uint32_t)c.cpb;
            psb[i] = a.sB + (long)min(n0 + wn * 64 + i * 16 + r, a.N - 1) * nblk;
        }
    }

    uint4 ra[NA];
    bool oka[NA];
    int sca[4], scb[4];
    if constexpr (I8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) sca[i] = scb[i] = 0;
    }
    int u_blk = 0, u_ts = 0, u_tr = 0;                               // where the next k tile to load starts
    if constexpr (SPLIT) {                                           // ... which is k tile kt0: once per workgroup
        const int b0 = 4 * kt0, tap = b0 / c.cpb;
        u_blk = b0 % c.cpb;
        u_tr = tap / c.kw;
        u_ts = tap % c.kw;
    }
    auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            int off, ts, tr;
            conv_tap_of(u_blk * (RA / 4) + ca[i], pbytes, u_ts, u_tr, c.kw, off, ts, tr);
            const int hi = hia[i] + tr * c.dh, wi = wia[i] + ts * c.dw;
            oka[i] = (tr < c.kh) & ((unsigned)hi < (unsigned)c.H) & ((unsigned)wi < (unsigned)c.W);    // tr >= kh: the K tail
            const uint32_t src = ga[i] + ((uint32_t)(tr * c.dh) * (uint32_t)c.W + (uint32_t)(ts * c.dw)) * (uint32_t)pbytes + (uint32_t)off;
            ra[i] = *(const uint4 *)(a.A + (oka[i] ? src : 0u));
        }
        B.load(kt);
        if constexpr (!I8) {
            int blk, ts, tr;
            conv_tap_of(u_blk + g, c.cpb, u_ts, u_tr, c.kw, blk, ts, tr);
            const uint32_t sdelta = ((uint32_t)(tr * c.dh) * (uint32_t)c.W + (uint32_t)(ts * c.dw)) * (uint32_t)c.cpb + (uint32_t)blk;
            const int kb = min(kt * 4 + g, nblk - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int hi = his[i] + tr * c.dh, wi = wis[i] + ts * c.dw;
                const bool ok = (tr < c.kh) & ((unsigned)hi < (unsigned)c.H) & ((unsigned)wi < (unsigned)c.W);
                const int sv = a.sA[ok ? gs[i] + sdelta : 0u];
                sca[i] = ok ? sv : 127;
                scb[i] = psb[i][kb];
            }
        }
        int nb, ns, nr;
        conv_tap_of(u_blk + 4, c.cpb, u_ts, u_tr, c.kw, nb, ns, nr);
        u_blk = nb; u_ts = ns; u_tr = nr;
    };
    auto store_tile = [&](int buf, int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NA; ++i) *(uint4 *)(s_a(buf) + la[i]) = chunk_or_zero(oka[i], ra[i]);
        B.store(s_b(buf), kt);
    };

    typename M_::acc_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = M_::zero();

    load_tile(kt0);
    store_tile(0, kt0);
    int cs_a[4], cs_b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { cs_a[i] = sca[i]; cs_b[i] = scb[i]; }
    __syncthreads();
    for (int kt = kt0; kt + 1 < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        load_tile(kt + 1);                                // in flight during this tile's MFMAs
        __builtin_amdgcn_sched_barrier(0);
        mma_tile<FA, FB, I8>(s_a(cur), s_b(cur), cs_a, cs_b, acc);
        __builtin_amdgcn_sched_barrier(0);
        store_tile(cur ^ 1, kt + 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) { cs_a[i] = sca[i]; cs_b[i] = scb[i]; }
        __syncthreads();
    }
    mma_tile<FA, FB, I8>(s_a((kt1 - 1 - kt0) & 1), s_b((kt1 - 1 - kt0) & 1), cs_a, cs_b, acc);

    if constexpr (SPLIT) {
        const v4i *const tile_ws = sp.ws + (long)id * sp.S * kSplitSlab;
        const v4i *const mine = tile_ws + (long)split * kSplitSlab;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) store16_sc1(mine + (i * 4 + j) * 256, (uint32_t)t * 16u, acc[i][j]);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                        // (also: every wave has read its last fragments, the flag reuses the tiles)
        volatile unsigned int *flag = (volatile unsigned int *)lds;
        if (t == 0) *flag = __hip_atomic_fetch_add(sp.tickets + id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if ((int)*flag != sp.S - 1) return;                     // not the last one: done
        if (t == 0) __hip_atomic_store(sp.tickets + id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // drop what this XCD's L2 holds of the workspace from earlier launches
#pragma unroll 1
        for (int q = 0; q < sp.S; ++q) {
            if (q == split) continue;
            v4i part[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[i][j] = load16_sc1(tile_ws + (long)q * kSplitSlab + (i * 4 + j) * 256, (uint32_t)t * 16u);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    asm volatile("" : "+v"(part[i][j]));
                    acc[i][j] += part[i][j];
                }
        }
    }

    // epilogue: D col = l & 15, row = 4 g + e; y is [M][Cout] = NHWC
    if constexpr (CODES) emit_codes_tile(a, ct, lds, acc, m0, n0, 0L);
    else emit_tile<I8>(a, acc, m0 + wm * 64, n0 + wn * 64, 0L, r, g);      // the float instantiations load no dequantize factor
}

template <int FA, int FB, bool I8 = false, bool CODES = false>
int launch_conv(const MxGemmArgs &g, const MxConvGeom &c, unsigned grid, hipStream_t st, const tail_t<CODES> &ct = {}) {
    constexpr int kLds = 2 * Tile<FA>::kBytes + 2 * Tile<FB>::kBytes;
    static_assert(!CODES || kBM * kCodePitch <= kLds, "the code tile is staged in the operand tiles' space");
    if (!I8 && g.out_scale) return QT_ERR_BAD_ARG;          // the float instantiations compile the dequantize factor out (emit_tile<false>)
    if (const int rc = qt_allow_lds<mx_conv_kernel<FA, FB, I8, CODES>>(kLds)) return rc;
    mx_conv_kernel<FA, FB, I8, CODES><<<grid, 256, kLds, st>>>(g, c, ct);
    return qt_launch_status();
}

// The split-K instantiations of the int8 kernel: grid = tiles * S work items.
template <bool CODES>
int launch_conv_split(const MxGemmArgs &g, const MxConvGeom &c, unsigned grid, hipStream_t st, const tail_t<CODES> &ct, const SplitK &sp) {
    constexpr int kLds = 4 * Tile<0>::kBytes;
    static_assert(!CODES || kBM * kCodePitch <= kLds, "the code tile is staged in the operand tiles' space");
    if (const int rc = qt_allow_lds<mx_conv_kernel<0, 0, true, CODES, true>>(kLds)) return rc;
    mx_conv_kernel<0, 0, true, CODES, true><<<grid, 256, kLds, st>>>(g, c, ct, sp);
    return qt_launch_status();
}

// ---- the plan of the split (qt_q8_conv2d_plan) ---------------------------------------------------------------------------------
// A fixed function of the shape and the CU count.  S = 1 once the 128 x 128 tiles give every CU a workgroup; else the largest
// S of kConvSplitSet with tiles * S <= CUs that leaves every split at least kConvSplitMinKTiles k tiles.  Both constants are read off
// profiles/conv2d_q_splitk.txt (MI355X, 256 CUs; the launch alone, replayed, us for S = 1 / 2 / 4 / 8 / 16):
//   * the set stops at 8: S = 16 is the slowest split wherever it was forced (2048 -> 512 at 7 x 7, 52 tiles, nk = 16:
//     37.6 / 31.9 / 30.4 / 35.6 / 50.0; 4 x 512 -> 512 3 x 3, 8 tiles, nk = 36: 61.3 / 42.5 / 33.6 / 32.7 / 38.9);
//   * at least two k tiles per split: one k tile each loses to the unsplit launch on every row (nk = 2, S = 2: 256 -> 64 at 56 x 56
//     39.6 -> 83.8, 192 -> 64 at 14 x 14 19.1 -> 21.5; nk = 8, S = 8: 960 -> 160 at 7 x 7 28.2 -> 30.3), two each is where the split
//     starts to pay (nk = 8, S = 4: 960 -> 160 28.2 -> 26.4, 960 -> 320 28.3 -> 27.4; nk = 5, S = 2: ties within about 1 us);
//   * tiles * S <= CUs: a second round of workgroups costs more than it hides (512 -> 128 at 28 x 28, 196 tiles: 24.1 / 31.7 / 52.5).
// On all seventeen rows the S this gives is the fastest measured one or within about 1 us of it.
constexpr int kConvSplitSet[] = {8, 4, 2};
constexpr int kConvSplitMinKTiles = 2;
struct ConvSplitPlan {
    long tiles;
    int nk, ksplit;
    size_t ws_bytes() const { return ksplit > 1 ? (size_t)tiles * ksplit * kSplitSlab * sizeof(v4i) : 0; }
    size_t tickets() const { return ksplit > 1 ? (size_t)tiles : 0; }
};
struct ConvSplitWs {             // what the *_ws entry points add to their siblings' arguments
    int ksplit;
    void *ws;
    size_t ws_bytes;
    uint32_t *tickets;
    size_t n_tickets;
};
ConvSplitPlan conv_split_plan(long m, long cout, long K) {
    ConvSplitPlan p{((m + kBM - 1) / kBM) * ((cout + kBN - 1) / kBN), (int)((K + kBK - 1) / kBK), 1};
    const long cus = qt_cu_count();
    if (p.tiles < 1 || p.tiles >= cus) return p;
    for (const int s : kConvSplitSet)
        if (p.tiles * s <= cus && p.nk / s >= kConvSplitMinKTiles) { p.ksplit = s; break; }
    return p;
}

// ---- depthwise conv2d on int8 codes (qt_q8_dwconv2d) ---------------------------------------------------------
// No matrix work: y[n, ho, wo, c] sums kh kw products of channel c alone.  A thread's unit is one 16-byte run of channels
// (one global_load_dwordx4 of NHWC codes per tap) of P consecutive output pixels; its 16 P sums stay in int32 registers
// (kh kw <= 1023: |sum| < 2^24, exact).  A workgroup owns a slab of up to 256 channels (a.N = C, c.cpb = C / 16 runs) and
// 256 / runs strips of pixels.  The weight arrives as stored, [C][kh kw] bytes: the slab's bytes of 16 taps at a time are
// sign-extended and transposed through LDS into [tap][quad of the run][run][4] int32 -- the 16 runs of a tap's quad fill one
// 256-byte bank row, so the ds_read_b128 of a wave (lanes of one run read one address) is conflict-free -- and every tap
// costs a thread four LDS reads for all its P pixels, one v_bfe_i32 and one v_mad_i32_i24 per product.
// A tap outside the plane loads nothing and adds nothing (the row and column tests are per pixel and per tap: no tap
// wraps into the next row or image); threads past the slab or past M run the loops (barriers) with no load and no store.
// The kernel is paced by its chain of dependent memory round trips (weight staging, the groups of taps, bias and factors,
// the stores: about 9 us for any workgroup, times the generations of workgroups), not by bytes or instructions: the codes of
// four taps are requested together and the next group before the current group's products are formed (against one tap in
// flight, MobileNetV2's layers at batch 32: 6 - 14 % less time where the kernel takes 14 us or more, 5 - 13 % more below).
constexpr int kDwSlab = 256, kDwRuns = kDwSlab / 16, kDwTaps = 16;

template <int P, bool CODES = false>
__global__ __launch_bounds__(256) void q8_dwconv_kernel(MxGemmArgs a, MxConvGeom c, tail_t<CODES> ct = {}) {
    __shared__ __attribute__((aligned(16))) int wl[kDwTaps * kDwSlab];
    const int C = a.N, taps = c.kh * c.kw;
    const int nslab = (C + kDwSlab - 1) / kDwSlab;
    const int slab = blockIdx.x % nslab, pb = blockIdx.x / nslab;
    const int c0 = slab * kDwSlab, cs = min(kDwSlab, C - c0);
    const int runs = min(c.cpb, kDwRuns);                  // of a full slab: the thread map is the same in the ragged last slab
    const int spb = 256 / runs;
    const int t = threadIdx.x, cg = t % runs, st = t / runs;
    const bool mine = cg * 16 < cs && st < spb;
    const long m0 = ((long)pb * spb + st) * P;
    const int8_t *x = (const int8_t *)a.A + c0 + cg * 16;

    int hi0[P], wi0[P];
    uint32_t img[P];                                       // pixel index of the image's first pixel
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const bool live = mine && m0 + p < a.M;
        const int mm = live ? (int)(m0 + p) : 0;
        const int n = mm / (c.Ho * c.Wo), rem = mm - n * (c.Ho * c.Wo), ho = rem / c.Wo, wo = rem - ho * c.Wo;
        hi0[p] = live ? ho * c.sh - c.ph : -(1 << 28);     // no tap (r dh < 2^20) brings a dead pixel back into the plane
        wi0[p] = wo * c.sw - c.pw;
        img[p] = (uint32_t)n * (uint32_t)(c.H * c.W);
    }
    // the codes of D consecutive taps from `first` on, for the P pixels: 4 P loads of 16 bytes requested together; (r, s) is the
    // tap `first` on entry and the tap behind the group on exit
    constexpr int D = 4;
    static_assert(kDwTaps % D == 0, "a group of taps never straddles two staging rounds");
    auto load_group = [&](int first, int &r, int &s, v4i (&v)[D][P]) __attribute__((always_inline)) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int p = 0; p < P; ++p) {
                const int hi = hi0[p] + r * c.dh, wi = wi0[p] + s * c.dw;
                v[d][p] = v4i{0, 0, 0, 0};
                if (first + d < taps && (unsigned)hi < (unsigned)c.H && (unsigned)wi < (unsigned)c.W)
                    v[d][p] = *(const v4i *)(x + (size_t)(img[p] + (uint32_t)hi * (uint32_t)c.W + (uint32_t)wi) * (size_t)C);
            }
            if (++s == c.kw) { s = 0; ++r; }
        }
    };

    int acc[P][16];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[p][i] = 0;
    int r = 0, s = 0;                                      // the tap whose codes are requested next
    v4i xn[D][P], xc[D][P];
    load_group(0, r, s, xn);
    for (int t0 = 0; t0 < taps; t0 += kDwTaps) {
        const int nt = min(kDwTaps, taps - t0);
        if (t0) __syncthreads();
        for (int e = t; e < cs * nt; e += 256) {           // consecutive threads: consecutive bytes of a channel's taps
            const int ch = e / nt, j = e - ch * nt;
            wl[((j * 4 + ((ch >> 2) & 3)) * kDwRuns + (ch >> 4)) * 4 + (ch & 3)] = ((const int8_t *)a.B)[(long)(c0 + ch) * taps + t0 + j];
        }
        __syncthreads();
        for (int j0 = 0; j0 < nt; j0 += D) {               // j0 + D <= kDwTaps
#pragma unroll
            for (int d = 0; d < D; ++d)
#pragma unroll
                for (int p = 0; p < P; ++p) xc[d][p] = xn[d][p];
            if (t0 + j0 + D < taps) load_group(t0 + j0 + D, r, s, xn);
#pragma unroll
            for (int d = 0; d < D; ++d) {
                if (j0 + d >= nt) break;                   // wave-uniform: the tail of the last group
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const v4i wq = *(const v4i *)&wl[(((j0 + d) * 4 + q) * kDwRuns + cg) * 4];
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const uint32_t v = (uint32_t)xc[d][p][q];
                        acc[p][4 * q + 0] += __mul24((int)(v << 24) >> 24, wq[0]);
                        acc[p][4 * q + 1] += __mul24((int)(v << 16) >> 24, wq[1]);
                        acc[p][4 * q + 2] += __mul24((int)(v << 8) >> 24, wq[2]);
                        acc[p][4 * q + 3] += __mul24((int)v >> 24, wq[3]);
                    }
                }
            }
        }
    }
    if (!mine) return;

    // epilogue: bias and factors of the run in 16-byte loads, the rounding chain of out_bits, the run's 32 or 64 bytes in 16-byte stores
    const int col = c0 + cg * 16;
    auto run16 = [&](const void *src, float (&out)[16]) __attribute__((always_inline)) {
        if (a.out_f32) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4f v = ((const v4f *)((const float *)src + col))[q];
#pragma unroll
                for (int k = 0; k < 4; ++k) out[4 * q + k] = v[k];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const v4i v = ((const v4i *)((const uint16_t *)src + col))[q];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    out[8 * q + 2 * k] = bf_lo((uint32_t)v[k]);
                    out[8 * q + 2 * k + 1] = bf_hi((uint32_t)v[k]);
                }
            }
        }
    };
    float bv[16], sv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) bv[i] = 0.f;
    if (a.bias) run16(a.bias, bv);
    if (a.out_scale && a.out_scale_per_col) run16(a.out_scale, sv);
    else {
        const float one = out_scale_of(a, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) sv[i] = one;
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
        if (m0 + p >= a.M) continue;
        if constexpr (CODES) {                             // the run's 16 codes of this pixel: one 16-byte store
            const float ns = next_scale_of(a, ct);
            uint32_t k[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 16; ++i) k[i >> 2] |= out_code(a, ct, ns, (float)acc[p][i], bv[i], sv[i]) << (8 * (i & 3));
            *(u32x4 *)((int8_t *)a.C + (m0 + p) * (long)C + col) = u32x4{k[0], k[1], k[2], k[3]};
            continue;
        }
        uint32_t o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = out_bits(a, (float)acc[p][i], bv[i], sv[i]);
        const long idx = (m0 + p) * (long)C + col;
        if (a.out_f32) {
            u32x4 *dst = (u32x4 *)((float *)a.C + idx);
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[q] = u32x4{o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]};
        } else {
            u32x4 *dst = (u32x4 *)((uint16_t *)a.C + idx);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                dst[q] = u32x4{o[8 * q] | (o[8 * q + 1] << 16), o[8 * q + 2] | (o[8 * q + 3] << 16), o[8 * q + 4] | (o[8 * q + 5] << 16),
                               o[8 * q + 6] | (o[8 * q + 7] << 16)};
        }
    }
}

// ---- the checked shape of a convolution launch ---------------------------------------------------------------------------------
// What qt_conv2d_mx, qt_q8_conv2d* and qt_q8_dwconv2d* check alike, in the order their callers see: the common argument errors; the
// caller's own verdict `rule_rc` (its channel rule and whatever else it reports for an empty output too); an empty output, which is
// QT_OK with nothing to launch; the alignment of the pointers or-ed into `ptrs`; the index limits -- 32-bit row and pixel indices,
// 32-bit byte offsets into the code arrays (x_pixel_bytes per input pixel, w_tap_bytes per output channel and tap), a contraction
// taps * kchan below 2^31; the output is indexed in 64 bits.
// (a product that reaches 2^31 saturates there, so that no argument can overflow the 64-bit arithmetic of the checks)
constexpr long kLim = 1L << 31;
long mul_sat(long a, long b) { return a >= kLim || b >= kLim ? kLim : (a * b >= kLim ? kLim : a * b); }

struct ConvShape {
    MxConvGeom c;                // cpb is the caller's
    long m, taps;                // output pixels N Ho Wo, filter taps kh kw
    bool empty;
};
int conv_shape(int N, int H, int W, int cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int rule_rc, uintptr_t ptrs,
               long kchan, long x_pixel_bytes, long w_tap_bytes, ConvShape &s) {
    s.empty = true;
    if (N < 0 || H < 1 || W < 1 || cout < 0) return QT_ERR_BAD_ARG;
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0) return QT_ERR_BAD_ARG;
    if (rule_rc) return rule_rc;
    const long eh = (long)H + 2L * ph - (long)dh * (kh - 1) - 1, ew = (long)W + 2L * pw - (long)dw * (kw - 1) - 1;
    if (N == 0 || cout == 0 || eh < 0 || ew < 0) return QT_OK;                                  // empty output: nothing to launch
    if (ptrs & 15u) return QT_ERR_UNALIGNED;
    const long ho = eh / sh + 1, wo = ew / sw + 1;
    s.m = mul_sat(N, mul_sat(ho, wo));
    s.taps = mul_sat(kh, kw);
    if (s.m >= kLim || mul_sat(s.taps, kchan) >= kLim || mul_sat(N, mul_sat(mul_sat(H, W), x_pixel_bytes)) >= kLim ||
        mul_sat(cout, mul_sat(s.taps, w_tap_bytes)) >= kLim || (long)kh * dh >= (1 << 20) || (long)kw * dw >= (1 << 20) ||
        ph >= (1 << 20) || pw >= (1 << 20) || sh >= (1 << 20) || sw >= (1 << 20))
        return QT_ERR_BAD_ARG;
    s.c = MxConvGeom{H, W, kh, kw, sh, sw, ph, pw, dh, dw, (int)ho, (int)wo, 0};
    s.empty = false;
    return QT_OK;
}

}  // namespace

extern "C" {

int qt_conv2d_mx(const uint8_t *x_codes, const uint8_t *x_e8m0, int x_format, const uint8_t *w_codes, const uint8_t *w_e8m0, int w_format,
                 void *y, int y_is_f32, const void *bias, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                 int pw, int dh, int dw, void *stream) {
    if (!x_codes || !x_e8m0 || !w_codes || !w_e8m0 || !y) return QT_ERR_BAD_ARG;
    if (x_format < 0 || x_format > 4 || w_format < 0 || w_format > 4) return QT_ERR_BAD_ARG;
    if (Cin < 32 || Cin % 32 != 0 || Cin > (1 << 24)) return QT_ERR_BAD_ARG;
    const long pbx = (long)Cin * elem_bits(x_format) / 8, pbw = (long)Cin * elem_bits(w_format) / 8;      // code bytes per pixel / tap
    const int rule_rc = !qt_pick_pair(MxPairs{}, x_format, w_format, [](auto) {}) ? QT_ERR_BAD_DTYPE                   // caller dequantizes
                                                                                   : (((pbx | pbw) & 15) ? QT_ERR_UNALIGNED : QT_OK);
    const uintptr_t ptrs = (uintptr_t)x_codes | (uintptr_t)x_e8m0 | (uintptr_t)w_codes | (uintptr_t)w_e8m0 | (uintptr_t)y | (uintptr_t)bias;
    ConvShape s;
    if (const int rc = conv_shape(N, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, rule_rc, ptrs, Cin, pbx, pbw, s)) return rc;
    if (s.empty) return QT_OK;
    const int K = (int)(s.taps * Cin);
    MxGemmArgs g{x_codes, w_codes, x_e8m0, w_e8m0, y, bias, (int)s.m, Cout, K, 0, 0, 0, 0, 0, y_is_f32, nullptr, 0, 0};
    s.c.cpb = Cin / 32;
    const long tiles = ((s.m + kBM - 1) / kBM) * ((Cout + kBN - 1) / kBN);
    if (tiles >= kLim) return QT_ERR_BAD_ARG;
    int rc = QT_ERR_BAD_DTYPE;
    qt_pick_pair(MxPairs{}, x_format, w_format, [&](auto P) {
        rc = launch_conv<decltype(P)::a, decltype(P)::b>(g, s.c, (unsigned)tiles, (hipStream_t)stream);
    });
    return rc;
}

static int q8_conv2d_launch(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                            int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                            int pw, int dh, int dw, void *stream, const CodesTail *ct, const ConvSplitWs *wsp = nullptr) {
    if (!x_codes || !w_codes || !y) return QT_ERR_BAD_ARG;
    if (wsp && wsp->ksplit < 0) return QT_ERR_BAD_ARG;
    if (ct) {
        if (const int rc = codes_tail_check(*ct, Cout < 0 ? 0 : Cout, y, y_is_f32)) return rc;
    }
    // Cin % 32: a 16-byte chunk never straddles a tap and a 128-byte k tile spans at most four taps beyond its first (conv_tap_of)
    // kh kw Cin < 2^17: |sum| <= (2^17 - 1) * 128 * 128 < 2^31, the int32 accumulator never wraps
    const long taps = kh < 1 || kw < 1 ? 0 : mul_sat(kh, kw);                                   // conv_shape rejects such a filter first
    const bool rule = Cin >= 32 && Cin % 32 == 0 && Cin <= (1 << 24) && mul_sat(taps, Cin) < (1L << 17);
    const uintptr_t ptrs = (uintptr_t)x_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)out_scale;
    ConvShape s;
    if (const int rc = conv_shape(N, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, rule ? QT_OK : QT_ERR_BAD_ARG, ptrs, Cin, Cin, Cin, s)) return rc;
    if (s.empty) return QT_OK;
    const long m = s.m;
    const int K = (int)(s.taps * Cin);
    const uint8_t *A = (const uint8_t *)x_codes, *B = (const uint8_t *)w_codes;
    MxGemmArgs g{A, B, nullptr, nullptr, y, bias, (int)m, Cout, K, 0, 0, 0, 0, 0, y_is_f32, out_scale, out_scale_per_col, fold_f32};
    s.c.cpb = Cin / 32;
    const MxConvGeom &c = s.c;
    const long tiles = ((m + kBM - 1) / kBM) * ((Cout + kBN - 1) / kBN);
    if (tiles >= kLim) return QT_ERR_BAD_ARG;
    if (wsp) {
        // ksplit 0: the plan's; an explicit value is honoured up to the k tiles there are; 1 is the unsplit launch below
        ConvSplitPlan p = conv_split_plan(m, Cout, K);
        if (wsp->ksplit > 0) p.ksplit = wsp->ksplit;
        if (p.ksplit > p.nk) return QT_ERR_BAD_ARG;
        if (p.ksplit > 1) {
            if (tiles * p.ksplit >= kLim) return QT_ERR_BAD_ARG;
            if (!wsp->ws || !wsp->tickets || wsp->ws_bytes < p.ws_bytes() || wsp->n_tickets < p.tickets()) return QT_ERR_BAD_ARG;
            if (((uintptr_t)wsp->ws & 15u) || ((uintptr_t)wsp->tickets & 3u)) return QT_ERR_UNALIGNED;
            const SplitK sp{(v4i *)wsp->ws, wsp->tickets, p.ksplit};
            const unsigned grid = (unsigned)(tiles * p.ksplit);
            if (ct) return launch_conv_split<true>(g, c, grid, (hipStream_t)stream, *ct, sp);
            return launch_conv_split<false>(g, c, grid, (hipStream_t)stream, NoTail{}, sp);
        }
    }
    if (ct) return launch_conv<0, 0, true, true>(g, c, (unsigned)tiles, (hipStream_t)stream, *ct);
    return launch_conv<0, 0, true>(g, c, (unsigned)tiles, (hipStream_t)stream);
}

int qt_q8_conv2d_plan(long M, int Cout, int K, int *ksplit, size_t *ws_bytes, size_t *n_tickets) {
    if (M < 0 || Cout < 0 || K < 32 || K % 32 != 0 || K >= (1 << 17) || M >= (1L << 31)) return QT_ERR_BAD_ARG;
    ConvSplitPlan p{0, 0, 1};
    if (M * Cout != 0) p = conv_split_plan(M, Cout, K);
    if (ksplit) *ksplit = p.ksplit;
    if (ws_bytes) *ws_bytes = p.ws_bytes();
    if (n_tickets) *n_tickets = p.tickets();
    return QT_OK;
}

int qt_q8_conv2d_ws(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                    int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                    int dh, int dw, int ksplit, void *ws, size_t ws_bytes, uint32_t *tickets, size_t n_tickets, void *stream) {
    const ConvSplitWs wsp{ksplit, ws, ws_bytes, tickets, n_tickets};
    return q8_conv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh, kw, sh, sw,
                            ph, pw, dh, dw, stream, nullptr, &wsp);
}

int qt_q8_conv2d_codes_ws(const int8_t *x_codes, const int8_t *w_codes, int8_t *y, int y_is_f32, const void *bias, const void *out_scale,
                          int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                          int pw, int dh, int dw, int act, float act_lo, float act_hi, const void *next_scale, const uint16_t *next_qmap,
                          int ksplit, void *ws, size_t ws_bytes, uint32_t *tickets, size_t n_tickets, void *stream) {
    const CodesTail ct{next_qmap, next_scale, act, act_lo, act_hi};
    const ConvSplitWs wsp{ksplit, ws, ws_bytes, tickets, n_tickets};
    return q8_conv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh, kw, sh, sw,
                            ph, pw, dh, dw, stream, &ct, &wsp);
}

int qt_q8_conv2d(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                 int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw,
                 int dh, int dw, void *stream) {
    return q8_conv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh, kw, sh, sw,
                            ph, pw, dh, dw, stream, nullptr);
}

int qt_q8_conv2d_codes(const int8_t *x_codes, const int8_t *w_codes, int8_t *y, int y_is_f32, const void *bias, const void *out_scale,
                       int out_scale_per_col, int fold_f32, int N, int H, int W, int Cin, int Cout, int kh, int kw, int sh, int sw, int ph,
                       int pw, int dh, int dw, int act, float act_lo, float act_hi, const void *next_scale, const uint16_t *next_qmap,
                       void *stream) {
    const CodesTail ct{next_qmap, next_scale, act, act_lo, act_hi};
    return q8_conv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, Cin, Cout, kh, kw, sh, sw,
                            ph, pw, dh, dw, stream, &ct);
}

static int q8_dwconv2d_launch(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                              int out_scale_per_col, int fold_f32, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                              int dh, int dw, void *stream, const CodesTail *ct) {
    if (!x_codes || !w_codes || !y) return QT_ERR_BAD_ARG;
    if (ct) {
        if (const int rc = codes_tail_check(*ct, C < 0 ? 0 : C, y, y_is_f32)) return rc;
    }
    // a thread's unit is one 16-byte run of channels (the rule of qt_quantize_codes_nhwc_*)
    // kh kw <= 1023: every partial sum has magnitude <= 1023 * 128 * 128 < 2^24, exact in int32 and in its conversion to fp32
    const bool rule = C >= 16 && C % 16 == 0 && C <= (1 << 24) && mul_sat(kh, kw) <= 1023;
    const uintptr_t ptrs = (uintptr_t)x_codes | (uintptr_t)w_codes | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)out_scale;
    ConvShape s;
    if (const int rc = conv_shape(N, H, W, C, kh, kw, sh, sw, ph, pw, dh, dw, rule ? QT_OK : QT_ERR_BAD_ARG, ptrs, 1, C, 1, s)) return rc;
    if (s.empty) return QT_OK;
    const long m = s.m;
    const uint8_t *A = (const uint8_t *)x_codes, *B = (const uint8_t *)w_codes;
    MxGemmArgs g{A, B, nullptr, nullptr, y, bias, (int)m, C, (int)s.taps, 0, 0, 0, 0, 0, y_is_f32, out_scale, out_scale_per_col, fold_f32};
    s.c.cpb = C / 16;
    const MxConvGeom &c = s.c;
    // two pixels per thread (half the LDS weight reads per product) once that still leaves two waves per SIMD of the chip
    const long runs = C / 16, spb = 256 / (runs < kDwRuns ? runs : kDwRuns), nslab = (C + kDwSlab - 1) / kDwSlab;
    const int P = m * runs >= 2L * 64 * 2048 ? 2 : 1;
    const long blocks = mul_sat(((m + P - 1) / P + spb - 1) / spb, nslab);
    if (blocks >= kLim) return QT_ERR_BAD_ARG;
    if (ct) qt_pick<1, 2>(P, [&](auto PP) { q8_dwconv_kernel<decltype(PP)::value, true><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(g, c, *ct); });
    else qt_pick<1, 2>(P, [&](auto PP) { q8_dwconv_kernel<decltype(PP)::value><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(g, c); });
    return qt_launch_status();
}

int qt_q8_dwconv2d(const int8_t *x_codes, const int8_t *w_codes, void *y, int y_is_f32, const void *bias, const void *out_scale,
                   int out_scale_per_col, int fold_f32, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                   int dh, int dw, void *stream) {
    return q8_dwconv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, C, kh, kw, sh, sw, ph, pw,
                              dh, dw, stream, nullptr);
}

int qt_q8_dwconv2d_codes(const int8_t *x_codes, const int8_t *w_codes, int8_t *y, int y_is_f32, const void *bias, const void *out_scale,
                         int out_scale_per_col, int fold_f32, int N, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                         int dh, int dw, int act, float act_lo, float act_hi, const void *next_scale, const uint16_t *next_qmap, void *stream) {
    const CodesTail ct{next_qmap, next_scale, act, act_lo, act_hi};
    return q8_dwconv2d_launch(x_codes, w_codes, y, y_is_f32, bias, out_scale, out_scale_per_col, fold_f32, N, H, W, C, kh, kw, sh, sw, ph, pw,
                              dh, dw, stream, &ct);
}

}  // extern "C"
