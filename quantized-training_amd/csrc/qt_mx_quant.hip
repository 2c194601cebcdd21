// Fused quantize_mx: one read of x, one write of the element values, the block scales, and -- when the element format is one
// the matrix instruction takes -- the packed operand for qt_mx_gemm.  quantize_mx_kernel takes blocks along the last axis,
// quantize_mx_strided_kernel blocks along any other axis (and, as the fake-quant entries, writes y = q * s instead of q).
//
// Replaces   quantize_mx(input, qmap, axes=[-1], block_size, quant_max, force_scale_power_of_two, scale_qmap)
//            decomposed.py:365-448  (calculate_mx_qparam: _reshape_to_blocks, _shared_exponents / amax, 2 ** e or
//            amax / quant_max [+ scale map], where(scale > 0, scale, 1);  quantize: input / expand(scale) -> vmap)
// which runs as a dozen elementwise / reduction passes in the reference, every op in the tensor's dtype.
//
// Shared exponent (mx_utils.py:19-55 with ebits = 0): floor(log2(amax + 2^-126 * (amax == 0))) with log2 evaluated
// in the tensor's dtype -- for bf16 that is bf16(log2f(amax)), whose rounding can reach the next integer (e.g.
// amax = 255 -> log2 = 7.994 -> bf16 8.0), so the floor is taken of the ROUNDED logarithm here as well.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/qt_hip.h"
#include "qt_device.h"
#include "qt_dispatch.h"
#include "qt_formats.h"
#include "qt_mx.h"
#include "qt_mx_log2_tables.h"

namespace {

struct MxQuantArgs {
    const uint4 *x;
    uint4 *q;                 // element values, tensor dtype (NULL = not wanted)
    void *sf;                 // block scales, tensor dtype, [rows][cols / bs]
    uint8_t *codes, *e8m0;    // packed operand (NULL = not wanted)
    size_t nvec;
    int group;                // lanes per block
    int lanes32;              // lanes per 32 elements (4 for bf16, 8 for fp32)
    qt_format fmt;
    const uint16_t *lut, *scale_lut;
    float quant_max;
    int qmax_exp;             // floor(log2(quant_max))
    int pow2, pack_fmt;
};

// The block scale (shared exponent, amax / quant_max, the where() guard) and the element codes of a vector are qt_mx.h's
// block_scale and vec_codes: this kernel and the strided one below call the same code.
//
// LDS_TABLE: the 128 KiB value map is staged in LDS once per workgroup (one 1024-thread workgroup per CU), so the
// per-element lookups are LDS reads instead of L2 gathers; worth it from a few million elements up.
// PACK_BITS: 0 = no packed operand, else the element width (8 / 6 / 4) -- compile-time so the packing is straight-line.
// ROWS: the value map in its row form (qt_format.p1 bit 0: the row words of qt_build_rowparams behind the map's 65 536 entries; csrc/qt_device.h
// Rounder<kFmtRows>): arithmetic against a 4 - 8 KiB row table in LDS instead of table gathers, at 256-thread occupancy.
template <int IO, bool LDS_TABLE, int PACK_BITS, bool ROWS = false>
__global__ __launch_bounds__(LDS_TABLE ? 1024 : 256) void quantize_mx_kernel(MxQuantArgs a) {
    constexpr int kThreads = LDS_TABLE ? 1024 : 256;
    static_assert(!(LDS_TABLE && ROWS), "one or the other");
    Rounder<kFmtRows> rnd{a.fmt, nullptr, a.lut};
    if constexpr (ROWS) {
        __shared__ uint4 s_rows[512];
        rnd = make_rounder<kFmtRows>(a.fmt, a.lut, s_rows, kThreads);
    }
    auto look = [&](uint32_t img) __attribute__((always_inline)) -> uint32_t {      // image of map[x]
        if constexpr (ROWS) return rnd(img);
        else return a.lut ? (uint32_t)a.lut[img >> 16] << 16 : qt_apply_format_img(a.fmt, img);
    };
    if constexpr (LDS_TABLE) {
        extern __shared__ __attribute__((aligned(16))) uint16_t s_table[];
        const uint4 *src = (const uint4 *)a.lut;
        uint4 *dst = (uint4 *)s_table;
#pragma unroll
        for (int i = 0; i < 65536 * 2 / 16 / kThreads; ++i) dst[threadIdx.x + i * kThreads] = src[threadIdx.x + i * kThreads];
        __syncthreads();
        a.lut = s_table;
    }
    const size_t stride = (size_t)gridDim.x * kThreads;
    const size_t iters = (a.nvec + stride - 1) / stride;
    for (size_t it = 0; it < iters; ++it) {
        const size_t v = it * stride + (size_t)blockIdx.x * kThreads + threadIdx.x;
        const bool live = v < a.nvec;
        uint4 in = {0u, 0u, 0u, 0u};
        if (live) in = a.x[v];
        const uint32_t w[4] = {in.x, in.y, in.z, in.w};
        uint32_t am = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (IO == kIoBf16) {
                const uint32_t a0 = (w[j] << 16) & 0x7FFFFFFFu, a1 = w[j] & 0x7FFF0000u;
                am = am > a0 ? am : a0;
                am = am > a1 ? am : a1;
            } else {
                const uint32_t a0 = w[j] & 0x7FFFFFFFu;
                am = am > a0 ? am : a0;
            }
        }
        for (int off = 1; off < a.group; off <<= 1) {       // block amax over `group` adjacent lanes; NaN patterns win
            const uint32_t o = (uint32_t)__shfl_xor((int)am, off, 64);
            am = am > o ? am : o;
        }
        const qt_mx::BlockScale sc = qt_mx::block_scale<IO>(am, a.pow2 != 0, a.quant_max, a.qmax_exp, a.scale_lut);
        const float s = sc.s;
        if (live && (threadIdx.x & (a.group - 1)) == 0) {
            const size_t blk = v / (size_t)a.group;
            if constexpr (IO == kIoBf16) ((uint16_t *)a.sf)[blk] = (uint16_t)(qt_f2u(s) >> 16);
            else ((float *)a.sf)[blk] = s;
        }
        // element values: map[x / s], every op in the tensor dtype
        const bool recip_ok = sc.recip_ok();
        const float r = sc.recip();
        constexpr int kPer = IO == kIoBf16 ? 8 : 4;
        float qv[kPer];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (IO == kIoBf16) {
                const float x0 = qt_u2f(w[j] << 16), x1 = qt_u2f(w[j] & 0xFFFF0000u);
                const uint32_t p = recip_ok ? pack_bf16x2(x0 * r, x1 * r) : pack_bf16x2(x0 / s, x1 / s);
                const uint32_t i0 = p << 16, i1 = p & 0xFFFF0000u;
                qv[2 * j] = qt_u2f(look(i0));
                qv[2 * j + 1] = qt_u2f(look(i1));
            } else {
                const float x0 = qt_u2f(w[j]);
                const uint32_t img = qt_fold_img(qt_f2u(recip_ok ? x0 * r : x0 / s));
                qv[j] = qt_u2f(look(img));
            }
        }
        if (!live) continue;
        if (a.q) {
            uint4 o;
            if constexpr (IO == kIoBf16) {
                o.x = (qt_f2u(qv[0]) >> 16) | (qt_f2u(qv[1]) & 0xFFFF0000u);
                o.y = (qt_f2u(qv[2]) >> 16) | (qt_f2u(qv[3]) & 0xFFFF0000u);
                o.z = (qt_f2u(qv[4]) >> 16) | (qt_f2u(qv[5]) & 0xFFFF0000u);
                o.w = (qt_f2u(qv[6]) >> 16) | (qt_f2u(qv[7]) & 0xFFFF0000u);
            } else {
                o.x = qt_f2u(qv[0]); o.y = qt_f2u(qv[1]); o.z = qt_f2u(qv[2]); o.w = qt_f2u(qv[3]);
            }
            a.q[v] = o;
        }
        if constexpr (PACK_BITS != 0) {
            constexpr int nbytes = kPer * PACK_BITS / 8;         // 8 / 6 / 4 (bf16) or 4 / 3 / 2 (fp32)
            uint8_t *dst = a.codes + v * (size_t)nbytes;
            qt_mx::VecCodes<PACK_BITS> vc = qt_mx::vec_codes<PACK_BITS>(qv, a.pack_fmt);
            if (sc.flush()) vc.w[0] = vc.w[1] = 0u;
            const uint32_t lo = vc.w[0], hi = vc.w[1];
            if constexpr (PACK_BITS == 8) {
                if constexpr (kPer == 8) *(uint2 *)dst = uint2{lo, hi};
                else *(uint32_t *)dst = lo;
            } else if constexpr (PACK_BITS == 4) {
                if constexpr (kPer == 8) *(uint32_t *)dst = lo;
                else *(uint16_t *)dst = (uint16_t)lo;
            } else {                                             // four codes in 24 bits
                if constexpr (kPer == 8) {
                    ((uint16_t *)dst)[0] = (uint16_t)lo;
                    ((uint16_t *)dst)[1] = (uint16_t)((lo >> 16) | (hi << 8));
                    ((uint16_t *)dst)[2] = (uint16_t)(hi >> 8);
                } else {
                    dst[0] = (uint8_t)lo; dst[1] = (uint8_t)(lo >> 8); dst[2] = (uint8_t)(lo >> 16);
                }
            }
            if ((threadIdx.x & (a.lanes32 - 1)) == 0) a.e8m0[v / (size_t)a.lanes32] = sc.e8m0();
        }
    }
}

template <int IO, int PB>
int launch_pb(const MxQuantArgs &a, bool rowform, bool lds, hipStream_t st) {
    const size_t want = (a.nvec + 255) / 256, cap = (size_t)qt_cu_count() * 32;
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    if (rowform) {                               // (8 workgroups per CU measured slower: 3.6 against 4.4 TB/s)
        quantize_mx_kernel<IO, false, PB, true><<<grid, 256, 0, st>>>(a);
    } else if (lds) {
        if (const int rc = qt_allow_lds<quantize_mx_kernel<IO, true, PB>>(65536 * 2)) return rc;
        quantize_mx_kernel<IO, true, PB><<<(unsigned)qt_cu_count(), 1024, 65536 * 2, st>>>(a);
    } else {
        quantize_mx_kernel<IO, false, PB><<<grid, 256, 0, st>>>(a);
    }
    return qt_launch_status();
}

template <int IO>
int launch(const void *x, void *q, void *sf, uint8_t *codes, uint8_t *e8m0, size_t rows, size_t cols, int bs,
           const qt_format *fmt, const uint16_t *lut, float quant_max, int pow2, const uint16_t *scale_lut, int pack_fmt,
           void *stream) {
    if (rows * cols == 0) return QT_OK;
    constexpr int kPer = IO == kIoBf16 ? 8 : 4;
    if (!x || !sf || !fmt || bs < kPer || (bs & (bs - 1)) || bs > 64 * kPer || !(quant_max > 0.0f)) return QT_ERR_BAD_ARG;
    if (fmt->kind == QT_FMT_LUT && !lut) return QT_ERR_BAD_ARG;
    if ((codes != nullptr) != (e8m0 != nullptr)) return QT_ERR_BAD_ARG;
    if (codes && (pack_fmt < 0 || pack_fmt > 4 || bs % 32 != 0 || !pow2)) return QT_ERR_BAD_ARG;
    if ((cols % (size_t)bs) || (((uintptr_t)x | (uintptr_t)q) & 15u)) return QT_ERR_UNALIGNED;
    int qe = 0;
    (void)frexpf(quant_max, &qe);                      // quant_max = m * 2^qe, m in [0.5, 1)  ->  floor(log2) = qe - 1
    MxQuantArgs a{(const uint4 *)x, (uint4 *)q, sf, codes, e8m0, rows * cols / kPer, bs / kPer, 32 / kPer, *fmt,
                  fmt->kind == QT_FMT_LUT ? lut : nullptr, scale_lut, quant_max, qe - 1, pow2, pack_fmt};
    const int pb = codes ? qt_mx::elem_bits(pack_fmt) : 0;
    const bool rowform = a.lut && (fmt->p1 & 1) && (((uintptr_t)a.lut) & 15u) == 0;
    const bool lds = !rowform && a.lut && rows * cols >= ((size_t)1 << 22) && (((uintptr_t)a.lut) & 15u) == 0;
    hipStream_t st = (hipStream_t)stream;
    int rc = QT_ERR_BAD_ARG;
    qt_pick<0, 8, 6, 4>(pb, [&](auto PB) { rc = launch_pb<IO, decltype(PB)::value>(a, rowform, lds, st); });
    return rc;
}

// ---- blocks along an axis that is not the last -----------------------------------------------------------------------------------------
// The tensor is contiguous [outer][n][inner] (ax=-2 on [B, H, S, D]: outer = B H, n = S, inner = D); a block is bs consecutive indices
// of n, the scales are [outer][n / bs][inner].  The work decomposition is fq_gwa_strided_kernel's (csrc/qt_groupwise.hip): a work item
// is one 16-byte column piece of one block, a workgroup is [G row groups][C = threads / G items], row group g keeps rows
// [g R, (g + 1) R) of the block in registers (R <= 8), the G partial amax vectors of an item meet in LDS behind one barrier, and every
// thread then derives the scales of its 8 (4) columns and quantizes the rows it holds: x is read once, whatever bs.
//
// Which items a workgroup takes:
//   no pack    items in memory order, pieces fastest (item m = (block, piece)): no dead lanes but in the last workgroup;
//   pack       a tile of PT pieces x NB blocks of the SAME columns (PT NB = C): the packed operand is written transposed,
//              codes [outer][inner][n bits / 8], so a column's codes of one block are only bs bits / 8 bytes of a code row.  The tile's
//              codes go to LDS one byte per element, column-major: column cl starts at cl (NB bs + 4) + (cl / K) 4 bytes.  A 32-lane
//              half of a wave writes one word each for 8 pieces x 4 blocks (bs = 32); ds_write banks are (a / 4) % 32, the blocks are
//              8 words apart and the pieces K (NB bs / 4 + 1) + 1 words, which is odd modulo 8: 32 different banks.  After one barrier
//              a thread takes 32 consecutive elements of one column -- 32 / 24 / 16 bytes of a code row and one E8M0 byte -- with
//              consecutive threads on consecutive pieces of the same code row: runs of NB bs bits / 8 bytes (256 at bs = 32, 8 bits).
// FQ: the fake-quant entry, y = rd(q * s) instead of q.
struct MxStridedArgs {
    const uint4 *x;
    uint4 *q;                 // q, or y of the fake-quant entries (NULL = not wanted)
    uint4 *sf;
    uint8_t *codes, *e8m0;    // packed operand (NULL = not wanted)
    size_t items;             // outer * nblk * P
    size_t ntiles;            // workgroups' worth of work
    size_t inner;
    size_t crow, erow;        // bytes of a code row (n bits / 8) and of an E8M0 row (n / 32)
    uint32_t P, nblk;         // 16-byte pieces of a row; blocks along n
    int bs, G, R;
    int PT, NB;               // pack: the tile, in pieces and in blocks
    uint32_t TP, TB;          // pack: tiles across the pieces and along the blocks of one `outer`
    qt_format fmt;
    const uint16_t *lut, *scale_lut;
    float quant_max;
    int qmax_exp;
    int pow2, pack_fmt;
};

constexpr int kMxRows = 8;

template <int IO, bool LDS_TABLE, int PACK_BITS, bool ROWS, bool FQ>
__global__ __launch_bounds__(LDS_TABLE ? 1024 : 256) void quantize_mx_strided_kernel(MxStridedArgs a) {
    constexpr int kThreads = LDS_TABLE ? 1024 : 256;
    constexpr int K = IO == kIoBf16 ? 8 : 4;
    static_assert(!(LDS_TABLE && (ROWS || PACK_BITS != 0)), "the 128 KiB table leaves no room for the pack tile");
    static_assert(!(FQ && PACK_BITS != 0), "the fake-quant entries have no packed operand");
    __shared__ uint4 s_part[kThreads];
    // pack: at most 256 * kMxRows * K elements of a tile, one byte each, + 4 bytes for each of its at most 8 K columns and 8 pieces
    __shared__ uint32_t s_tile[PACK_BITS != 0 ? (256 * kMxRows * K + 4 * 8 * K + 4 * 8) / 4 : 1];
    __shared__ uint8_t s_e8[PACK_BITS != 0 ? 64 * K : 1];            // [NB][PT K]: C <= 64 when bs >= 32
    Rounder<kFmtRows> rnd{a.fmt, nullptr, a.lut};
    if constexpr (ROWS) {
        __shared__ uint4 s_rows[512];
        rnd = make_rounder<kFmtRows>(a.fmt, a.lut, s_rows, kThreads);
    }
    extern __shared__ __attribute__((aligned(16))) uint16_t s_table[];
    if constexpr (LDS_TABLE) {
        stage_map<kThreads>(a.lut, (uint4 *)s_table);
        __syncthreads();
    }
    auto look = [&](uint32_t img) __attribute__((always_inline)) -> uint32_t {      // image of map[x]
        if constexpr (ROWS) return rnd(img);
        else if constexpr (LDS_TABLE) return (uint32_t)s_table[img >> 16] << 16;
        else return a.lut ? (uint32_t)a.lut[img >> 16] << 16 : qt_apply_format_img(a.fmt, img);
    };
    const int C = kThreads / a.G;
    const int c = threadIdx.x & (C - 1), g = threadIdx.x / C;
    const int r0 = g * a.R;
    for (size_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {       // one trip, but for LDS_TABLE (one workgroup per CU)
        size_t ob;                                                    // block, counted through [outer][n / bs]
        uint32_t p;                                                   // piece of the row
        bool live;
        [[maybe_unused]] size_t o = 0;
        [[maybe_unused]] uint32_t tb = 0, tp = 0, kbl = 0, pl = 0;    // the tile; block and piece within it
        if constexpr (PACK_BITS != 0) {
            const size_t per_o = (size_t)a.TB * a.TP;
            o = t / per_o;
            const uint32_t rem = (uint32_t)(t - o * per_o);
            tb = rem / a.TP;
            tp = rem - tb * a.TP;
            pl = (uint32_t)c & (uint32_t)(a.PT - 1);
            kbl = (uint32_t)c / (uint32_t)a.PT;
            const uint32_t kb = tb * (uint32_t)a.NB + kbl;
            p = tp * (uint32_t)a.PT + pl;
            live = kb < a.nblk && p < a.P;
            ob = o * a.nblk + kb;
        } else {
            const size_t m = t * (size_t)C + (size_t)c;
            live = m < a.items;
            ob = m / a.P;
            p = (uint32_t)(m - ob * a.P);
        }
        const size_t base = ob * (size_t)a.bs * a.P + p;              // vector index of row 0 of the block, this piece
        const int nrows = live ? min(a.R, a.bs - r0) : 0;             // may be <= 0 in the last row groups
        const uint4 *xr = a.x + base + (size_t)r0 * a.P;
        uint4 d[kMxRows];
#pragma unroll
        for (int j = 0; j < kMxRows; ++j)
            if (j < nrows) d[j] = xr[(size_t)j * a.P];
        // amax per column on absolute bit patterns (NaN patterns win); bf16: two 16-bit patterns to a word
        uint32_t amw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < kMxRows; ++j) {
            if (j < nrows) {
                const uint32_t w[4] = {d[j].x, d[j].y, d[j].z, d[j].w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (IO == kIoBf16) amw[i] = pk_max_u16(amw[i], w[i] & 0x7FFF7FFFu);
                    else amw[i] = max(amw[i], w[i] & 0x7FFFFFFFu);
                }
            }
        }
        if (a.G > 1) {                                                // uniform: the partial results of the G row groups meet in LDS
            s_part[threadIdx.x] = uint4{amw[0], amw[1], amw[2], amw[3]};
            __syncthreads();
            for (int gg = 0; gg < a.G; ++gg) {
                if (gg == g) continue;
                const uint4 o4 = s_part[gg * C + c];
                const uint32_t w[4] = {o4.x, o4.y, o4.z, o4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if constexpr (IO == kIoBf16) amw[i] = pk_max_u16(amw[i], w[i]);
                    else amw[i] = max(amw[i], w[i]);
                }
            }
        }
        qt_mx::BlockScale sc[K];
        bool all_recip = true;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            uint32_t am;
            if constexpr (IO == kIoBf16) am = (e & 1) ? (amw[e >> 1] & 0xFFFF0000u) : (amw[e >> 1] << 16);
            else am = amw[e];
            sc[e] = qt_mx::block_scale<IO>(am, a.pow2 != 0, a.quant_max, a.qmax_exp, a.scale_lut);
            all_recip &= sc[e].recip_ok();
        }
        if (live && g == 0) {
            uint4 o4;
            if constexpr (IO == kIoBf16) {
                o4.x = (qt_f2u(sc[0].s) >> 16) | (qt_f2u(sc[1].s) & 0xFFFF0000u);
                o4.y = (qt_f2u(sc[2].s) >> 16) | (qt_f2u(sc[3].s) & 0xFFFF0000u);
                o4.z = (qt_f2u(sc[4].s) >> 16) | (qt_f2u(sc[5].s) & 0xFFFF0000u);
                o4.w = (qt_f2u(sc[6].s) >> 16) | (qt_f2u(sc[7].s) & 0xFFFF0000u);
            } else {
                o4 = uint4{qt_f2u(sc[0].s), qt_f2u(sc[1].s), qt_f2u(sc[2].s), qt_f2u(sc[3].s)};
            }
            a.sf[ob * a.P + p] = o4;
        }
        if (a.q || PACK_BITS != 0) {                                  // uniform; scales only otherwise
            // element values: map[x / s], every op in the tensor dtype; x * 2^-se where that is x / s exactly
            [[maybe_unused]] uint32_t clo[K], chi[K];                 // pack: a column's codes of rows 0-3 and 4-7, a byte each
            if constexpr (PACK_BITS != 0) {
#pragma unroll
                for (int e = 0; e < K; ++e) clo[e] = chi[e] = 0u;
            }
            uint4 *qr = a.q + base + (size_t)r0 * a.P;
#pragma unroll
            for (int j = 0; j < kMxRows; ++j) {
                if (j < nrows) {
                    const uint32_t w[4] = {d[j].x, d[j].y, d[j].z, d[j].w};
                    float qv[K];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if constexpr (IO == kIoBf16) {
                            const float x0 = bf_lo(w[i]), x1 = bf_hi(w[i]);
                            const uint32_t pq = all_recip ? pack_bf16x2(x0 * sc[2 * i].recip(), x1 * sc[2 * i + 1].recip())
                                                          : pack_bf16x2(x0 / sc[2 * i].s, x1 / sc[2 * i + 1].s);
                            qv[2 * i] = qt_u2f(look(pq << 16));
                            qv[2 * i + 1] = qt_u2f(look(pq & 0xFFFF0000u));
                        } else {
                            const float x0 = qt_u2f(w[i]);
                            qv[i] = qt_u2f(look(qt_fold_img(qt_f2u(all_recip ? x0 * sc[i].recip() : x0 / sc[i].s))));
                        }
                    }
                    if (a.q) {
                        uint4 o4;
                        if constexpr (FQ) {                           // y = rd(q * s)
                            if constexpr (IO == kIoBf16)
                                o4 = uint4{pack_bf16x2(qv[0] * sc[0].s, qv[1] * sc[1].s), pack_bf16x2(qv[2] * sc[2].s, qv[3] * sc[3].s),
                                           pack_bf16x2(qv[4] * sc[4].s, qv[5] * sc[5].s), pack_bf16x2(qv[6] * sc[6].s, qv[7] * sc[7].s)};
                            else
                                o4 = uint4{qt_f2u(qv[0] * sc[0].s), qt_f2u(qv[1] * sc[1].s), qt_f2u(qv[2] * sc[2].s), qt_f2u(qv[3] * sc[3].s)};
                        } else if constexpr (IO == kIoBf16) {
                            o4.x = (qt_f2u(qv[0]) >> 16) | (qt_f2u(qv[1]) & 0xFFFF0000u);
                            o4.y = (qt_f2u(qv[2]) >> 16) | (qt_f2u(qv[3]) & 0xFFFF0000u);
                            o4.z = (qt_f2u(qv[4]) >> 16) | (qt_f2u(qv[5]) & 0xFFFF0000u);
                            o4.w = (qt_f2u(qv[6]) >> 16) | (qt_f2u(qv[7]) & 0xFFFF0000u);
                        } else {
                            o4 = uint4{qt_f2u(qv[0]), qt_f2u(qv[1]), qt_f2u(qv[2]), qt_f2u(qv[3])};
                        }
                        qr[(size_t)j * a.P] = o4;
                    }
                    if constexpr (PACK_BITS != 0) {
                        const qt_mx::VecCodes<PACK_BITS> vc = qt_mx::vec_codes<PACK_BITS>(qv, a.pack_fmt);
#pragma unroll
                        for (int e = 0; e < K; ++e) {
                            const uint32_t code = sc[e].flush() ? 0u : vc.code(e);
                            if (j < 4) clo[e] |= code << (8 * j);
                            else chi[e] |= code << (8 * (j - 4));
                        }
                    }
                }
            }
            if constexpr (PACK_BITS != 0) {
                const int NT = a.NB * a.bs, S = NT + 4, NCOL = a.PT * K;
                uint8_t *tile = (uint8_t *)s_tile;
                if (nrows > 0) {
                    const int at = (int)(pl * K) * S + (int)pl * 4 + (int)kbl * a.bs + r0;   // column pl K, this thread's first row
#pragma unroll
                    for (int e = 0; e < K; ++e) {
                        if (nrows == kMxRows && (r0 & 3) == 0) {                   // word-aligned: S and bs are multiples of 4
                            uint32_t *dst = (uint32_t *)(tile + at + e * S);
                            dst[0] = clo[e];
                            dst[1] = chi[e];
                        } else {
#pragma unroll
                            for (int j = 0; j < kMxRows; ++j)
                                if (j < nrows) tile[at + e * S + j] = (uint8_t)((j < 4 ? clo[e] : chi[e]) >> (8 * (j & 3)));
                        }
                    }
                    if (g == 0) {
#pragma unroll
                        for (int e = 0; e < K; ++e) s_e8[(int)kbl * NCOL + (int)(pl * K) + e] = sc[e].e8m0();
                    }
                }
                __syncthreads();
                const int UPR = NT / 32;                                           // 32-element units of a tile's code row
                const int units = NCOL * UPR;
                for (int u = threadIdx.x; u < units; u += kThreads) {
                    const int cl = u / UPR, ul = u - cl * UPR;
                    const size_t col = (size_t)tp * (size_t)NCOL + (size_t)cl;
                    const size_t n32 = (size_t)tb * (size_t)UPR + (size_t)ul;
                    if (col >= a.inner || n32 >= a.erow) continue;
                    const uint32_t *src = (const uint32_t *)(tile + cl * S + (cl / K) * 4 + ul * 32);
                    uint32_t b[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) b[i] = src[i];
                    const size_t row = o * a.inner + col;
                    uint8_t *dst = a.codes + row * a.crow + n32 * (size_t)(4 * PACK_BITS);
                    if constexpr (PACK_BITS == 8) {
                        ((uint4 *)dst)[0] = uint4{b[0], b[1], b[2], b[3]};
                        ((uint4 *)dst)[1] = uint4{b[4], b[5], b[6], b[7]};
                    } else if constexpr (PACK_BITS == 4) {
                        uint32_t h[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            h[i] = (b[i] & 0xFu) | ((b[i] >> 4) & 0xF0u) | ((b[i] >> 8) & 0xF00u) | ((b[i] >> 12) & 0xF000u);
                        *(uint4 *)dst = uint4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
                    } else {                                                       // 4 values to 3 bytes; a unit starts on 8 bytes
                        uint32_t h[8];
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            h[i] = (b[i] & 0x3Fu) | ((b[i] >> 2) & 0xFC0u) | ((b[i] >> 4) & 0x3F000u) | ((b[i] >> 6) & 0xFC0000u);
                        const uint32_t w0 = h[0] | (h[1] << 24), w1 = (h[1] >> 8) | (h[2] << 16), w2 = (h[2] >> 16) | (h[3] << 8);
                        const uint32_t w3 = h[4] | (h[5] << 24), w4 = (h[5] >> 8) | (h[6] << 16), w5 = (h[6] >> 16) | (h[7] << 8);
                        ((uint2 *)dst)[0] = uint2{w0, w1};
                        ((uint2 *)dst)[1] = uint2{w2, w3};
                        ((uint2 *)dst)[2] = uint2{w4, w5};
                    }
                    a.e8m0[row * a.erow + n32] = s_e8[((ul * 32) / a.bs) * NCOL + cl];
                }
            }
        }
        if constexpr (LDS_TABLE) __syncthreads();                     // s_part is written again in the next trip
    }
}

template <int IO, int PB, bool FQ>
int launch_strided_pb(const MxStridedArgs &a, bool rowform, bool lds, hipStream_t st) {
    if constexpr (PB == 0) {
        if (lds) {
            constexpr auto kernel = quantize_mx_strided_kernel<IO, true, 0, false, FQ>;
            if (const int rc = qt_allow_lds<kernel>(65536 * 2)) return rc;
            const size_t cus = (size_t)qt_cu_count();
            kernel<<<(unsigned)(a.ntiles < cus ? a.ntiles : cus), 1024, 65536 * 2, st>>>(a);
            return qt_launch_status();
        }
    }
    if (rowform) quantize_mx_strided_kernel<IO, false, PB, true, FQ><<<(unsigned)a.ntiles, 256, 0, st>>>(a);
    else quantize_mx_strided_kernel<IO, false, PB, false, FQ><<<(unsigned)a.ntiles, 256, 0, st>>>(a);
    return qt_launch_status();
}

inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// Every decline comes before the first HIP call or device query.
template <int IO, bool FQ>
int launch_strided(const void *x, void *q, void *sf, uint8_t *codes, uint8_t *e8m0, size_t outer, size_t n, size_t inner, int bs,
                   const qt_format *fmt, const uint16_t *lut, float quant_max, int pow2, const uint16_t *scale_lut, int pack_fmt,
                   void *stream) {
    if (outer * n * inner == 0) return QT_OK;
    constexpr int K = IO == kIoBf16 ? 8 : 4;
    if (!x || !sf || !fmt || (FQ && !q) || !(quant_max > 0.0f)) return QT_ERR_BAD_ARG;
    if (fmt->kind == QT_FMT_LUT && !lut) return QT_ERR_BAD_ARG;
    if ((codes != nullptr) != (e8m0 != nullptr)) return QT_ERR_BAD_ARG;
    const bool pack = codes != nullptr;
    if (bs < 1 || bs > 512) return QT_ERR_BAD_ARG;
    if (pack && (pack_fmt < 0 || pack_fmt > 4 || bs % 32 != 0 || !pow2)) return QT_ERR_BAD_ARG;
    if (inner == 1) return QT_ERR_BAD_ARG;                    // the last-axis layout: qt_quantize_mx_* / qt_fake_quant_mx_*
    if (inner / K > 0xFFFFFFFFull || n / (size_t)bs > 0xFFFFFFFFull) return QT_ERR_BAD_ARG;
    if (n % (size_t)bs || inner % K) return QT_ERR_UNALIGNED;  // the composite zero-pads, and the pad takes part in the amax
    if (!aligned16(x) || !aligned16(q) || !aligned16(sf) || !aligned16(codes) || !aligned16(e8m0)) return QT_ERR_UNALIGNED;
    const int pb = pack ? qt_mx::elem_bits(pack_fmt) : 0;
    if (pack && (n * (size_t)pb / 8) % 16) return QT_ERR_UNALIGNED;
    int qe = 0;
    (void)frexpf(quant_max, &qe);                             // quant_max = m * 2^qe, m in [0.5, 1)  ->  floor(log2) = qe - 1
    MxStridedArgs a{};
    a.x = (const uint4 *)x; a.q = (uint4 *)q; a.sf = (uint4 *)sf; a.codes = codes; a.e8m0 = e8m0;
    a.inner = inner; a.crow = n * (size_t)pb / 8; a.erow = n / 32;
    a.P = (uint32_t)(inner / K); a.nblk = (uint32_t)(n / (size_t)bs);
    a.items = outer * (size_t)a.nblk * a.P;
    a.bs = bs;
    a.fmt = *fmt; a.lut = fmt->kind == QT_FMT_LUT ? lut : nullptr; a.scale_lut = scale_lut;
    a.quant_max = quant_max; a.qmax_exp = qe - 1; a.pow2 = pow2; a.pack_fmt = pack_fmt;
    const bool rowform = a.lut && (fmt->p1 & 1) && aligned16(a.lut);
    const bool lds = !pack && !rowform && a.lut && outer * n * inner >= ((size_t)1 << 22) && aligned16(a.lut);
    const int threads = lds ? 1024 : 256;
    a.G = 1;
    while (a.G * kMxRows < bs) a.G <<= 1;                     // 1 .. 64 row groups
    a.R = (bs + a.G - 1) / a.G;
    const int C = threads / a.G;
    if (pack) {                                               // bs >= 32: G >= 4, C <= 64
        a.PT = C < 8 ? C : 8;                                 // 128 bytes of a row where the row has them
        while (a.PT > 1 && (uint32_t)(a.PT / 2) >= a.P) a.PT >>= 1;
        a.NB = C / a.PT;
        a.TP = (a.P + (uint32_t)a.PT - 1) / (uint32_t)a.PT;
        a.TB = (a.nblk + (uint32_t)a.NB - 1) / (uint32_t)a.NB;
        a.ntiles = outer * (size_t)a.TB * a.TP;
        if ((size_t)a.TB * a.TP > 0xFFFFFFFFull) return QT_ERR_BAD_ARG;
    } else {
        a.ntiles = (a.items + (size_t)C - 1) / (size_t)C;
    }
    if (a.ntiles > 0x7FFFFFFFull) return QT_ERR_BAD_ARG;
    hipStream_t st = (hipStream_t)stream;
    int rc = QT_ERR_BAD_ARG;
    if constexpr (FQ) rc = launch_strided_pb<IO, 0, true>(a, rowform, lds, st);
    else qt_pick<0, 8, 6, 4>(pb, [&](auto PB) { rc = launch_strided_pb<IO, decltype(PB)::value, false>(a, rowform, lds, st); });
    return rc;
}

}  // namespace

extern "C" {

int qt_quantize_mx_bf16(const uint16_t *x, uint16_t *q, uint16_t *scales, uint8_t *codes, uint8_t *e8m0, size_t rows,
                        size_t cols, int block_size, const qt_format *fmt, const uint16_t *lut, float quant_max,
                        int force_pow2, const uint16_t *scale_lut, int pack_format, void *stream) {
    return launch<kIoBf16>(x, q, scales, codes, e8m0, rows, cols, block_size, fmt, lut, quant_max, force_pow2, scale_lut,
                           pack_format, stream);
}

int qt_quantize_mx_f32(const float *x, float *q, float *scales, uint8_t *codes, uint8_t *e8m0, size_t rows, size_t cols,
                       int block_size, const qt_format *fmt, const uint16_t *lut, float quant_max, int force_pow2,
                       const uint16_t *scale_lut, int pack_format, void *stream) {
    return launch<kIoF32>(x, q, scales, codes, e8m0, rows, cols, block_size, fmt, lut, quant_max, force_pow2, scale_lut,
                          pack_format, stream);
}

int qt_quantize_mx_strided_bf16(const uint16_t *x, uint16_t *q, uint16_t *scales, uint8_t *codes, uint8_t *e8m0, size_t outer, size_t n,
                                size_t inner, int block_size, const qt_format *fmt, const uint16_t *lut, float quant_max, int force_pow2,
                                const uint16_t *scale_lut, int pack_format, void *stream) {
    return launch_strided<kIoBf16, false>(x, q, scales, codes, e8m0, outer, n, inner, block_size, fmt, lut, quant_max, force_pow2, scale_lut,
                                          pack_format, stream);
}

int qt_quantize_mx_strided_f32(const float *x, float *q, float *scales, uint8_t *codes, uint8_t *e8m0, size_t outer, size_t n, size_t inner,
                               int block_size, const qt_format *fmt, const uint16_t *lut, float quant_max, int force_pow2,
                               const uint16_t *scale_lut, int pack_format, void *stream) {
    return launch_strided<kIoF32, false>(x, q, scales, codes, e8m0, outer, n, inner, block_size, fmt, lut, quant_max, force_pow2, scale_lut,
                                         pack_format, stream);
}

int qt_fake_quant_mx_strided_bf16(const uint16_t *x, uint16_t *y, uint16_t *sf, size_t outer, size_t n, size_t inner, int block_size,
                                  const qt_format *fmt, const uint16_t *lut, float quant_max, int force_pow2, const uint16_t *scale_lut,
                                  void *stream) {
    return launch_strided<kIoBf16, true>(x, y, sf, nullptr, nullptr, outer, n, inner, block_size, fmt, lut, quant_max, force_pow2, scale_lut, 0,
                                         stream);
}

int qt_fake_quant_mx_strided_f32(const float *x, float *y, float *sf, size_t outer, size_t n, size_t inner, int block_size,
                                 const qt_format *fmt, const uint16_t *lut, float quant_max, int force_pow2, const uint16_t *scale_lut,
                                 void *stream) {
    return launch_strided<kIoF32, true>(x, y, sf, nullptr, nullptr, outer, n, inner, block_size, fmt, lut, quant_max, force_pow2, scale_lut, 0,
                                        stream);
}

}  // extern "C"
