// qt_outlier.hip -- the outlier side path of a block-scaled linear layer (upstream decomposed.py:450-566): filter_outlier as three
// launches without a host read, and spmm_csr as one launch that takes the stored weight in place.
//
// filter_outlier, x [R][C] contiguous:
//   1. outlier_split_kernel    one wave per row: reads the row once, writes the inlier and the row's entry count into indptr[r + 1]
//   2. outlier_scan_kernel     ONE workgroup turns the counts into indptr in place (chunks of kScanChunk rows, a carry in registers)
//   3. outlier_compact_kernel  one wave per row with entries: reads the row again (L2), ranks its entries with one ballot per vector
//                              slot and the count of set bits below the lane, stores the first max_nnz; the grid zeroes the padding
//   No workgroup waits for another one: the three phases are ordered by the stream alone.
//
// spmm_csr, Y[r][n] = sum_i data[i] Bd[n][indices[i]]: a workgroup owns TN output features.  It stages their TN rows of the
// operand -- codebook lookup and block scale applied, rounded to the tensor's dtype exactly as the composite's `B_code[B] * expand(scale)`
// -- into LDS as tile[k][TN], so that the weight is read from memory once per launch and coalesced in either stored layout; no
// dequantized, gathered or transposed copy goes back to memory.  Then one THREAD per CSR row walks the row's entries in order: one LDS
// read of TN values and TN fused multiply-adds per entry, fp32 accumulators, one rounding, every Y element written.  The order of a
// sum is fixed -- the row's entries in order, in groups of 16 whose sums are added in order --: no atomics, the same bits on every launch.
#include "qt_device.h"

namespace {

template <int IO> struct ElemOf { using type = uint16_t; };
template <> struct ElemOf<kIoF32> { using type = uint32_t; };

template <int IO>
__device__ __forceinline__ float elem_f(typename ElemOf<IO>::type b) {
    if constexpr (IO == kIoBf16) return qt_u2f((uint32_t)b << 16);
    else return qt_u2f(b);
}
// fp32 -> the tensor's dtype, round to nearest even (torch's cast)
template <int IO>
__device__ __forceinline__ typename ElemOf<IO>::type elem_of(float f) {
    if constexpr (IO == kIoBf16) return (uint16_t)(pack_bf16x2(f, 0.0f) & 0xFFFFu);
    else return qt_f2u(f);
}

__host__ __device__ inline bool aligned16(const void *p) { return (((uintptr_t)p) & 15u) == 0; }

// ---- filter_outlier ----------------------------------------------------------------------------------------------------------------------
constexpr int kRowWaves = 4;                 // waves (rows in flight) per workgroup of the two row passes
constexpr int kScanThreads = 1024;
constexpr int kScanChunk = kScanThreads * 4;   // rows one sweep of the scan covers

// One row in wave-sized steps, in column order: the <= VEC - 1 elements in front of the first 16-byte boundary (one per lane), the
// aligned body (VEC consecutive elements per lane and sweep), the tail (one per lane).  f(first column, count 0..VEC, values) is
// called by all 64 lanes in every step (it may hold wave-wide operations); the values as it leaves them are stored to `out` (nullable).
template <int IO, class F>
__device__ __forceinline__ void walk_row(const typename ElemOf<IO>::type *__restrict__ row, typename ElemOf<IO>::type *__restrict__ out, long C,
                                         int lane, F &&f) {
    using E = typename ElemOf<IO>::type;
    constexpr int VEC = 16 / (int)sizeof(E);
    long head = (long)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) / sizeof(E));
    head = head < C ? head : C;
    const long nvec = (C - head) / VEC;
    const long tail0 = head + nvec * VEC;
    E e[VEC];
    auto single = [&](long c0, long n) __attribute__((always_inline)) {
        const bool mine = lane < n;
        if (mine) e[0] = row[c0 + lane];
        f(c0 + lane, mine ? 1 : 0, e);
        if (out && mine) out[c0 + lane] = e[0];
    };
    if (head) single(0, head);
    const bool vst = out && aligned16(out + head);
    for (long v0 = 0; v0 < nvec; v0 += 64) {
        const long v = v0 + lane;
        const bool mine = v < nvec;
        const long c0 = head + v * VEC;
        if (mine) {
            const uint4 q = *(const uint4 *)(row + c0);
            __builtin_memcpy(e, &q, 16);
        }
        f(c0, mine ? VEC : 0, e);
        if (out && mine) {
            if (vst) {
                uint4 q;
                __builtin_memcpy(&q, e, 16);
                *(uint4 *)(out + c0) = q;
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) out[c0 + j] = e[j];
            }
        }
    }
    if (tail0 < C) single(tail0, C - tail0);
}

// bit j of the result: element j is a CSR entry (|x| > threshold and x != 0; a NaN compares false).  Outliers become +0 in e.
template <int IO, int VEC>
__device__ __forceinline__ uint32_t split_values(typename ElemOf<IO>::type (&e)[VEC], int n, float thr) {
    uint32_t entries = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        if (j < n) {
            const float x = elem_f<IO>(e[j]);
            if (__builtin_fabsf(x) > thr) {
                e[j] = 0;
                entries |= (x != 0.0f ? 1u : 0u) << j;
            }
        }
    }
    return entries;
}

template <int IO>
__global__ __launch_bounds__(kRowWaves * 64) void outlier_split_kernel(const typename ElemOf<IO>::type *__restrict__ x,
                                                                       typename ElemOf<IO>::type *__restrict__ inlier, int32_t *__restrict__ indptr,
                                                                       long R, long C, float thr) {
    using E = typename ElemOf<IO>::type;
    constexpr int VEC = 16 / (int)sizeof(E);
    const int lane = threadIdx.x & 63;
    const long nw = (long)gridDim.x * kRowWaves;
    for (long r = (long)blockIdx.x * kRowWaves + (threadIdx.x >> 6); r < R; r += nw) {
        int count = 0;
        walk_row<IO>(x + r * C, inlier + r * C, C, lane, [&](long, int n, E(&e)[VEC]) __attribute__((always_inline)) {
            count += __builtin_popcount(split_values<IO, VEC>(e, n, thr));
        });
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) count += __shfl_xor(count, off, 64);
        if (lane == 0) indptr[r + 1] = count;
    }
}

// indptr[1 ..R] holds the rows' counts -> their inclusive prefix sums; indptr[0] = 0.  One workgroup: nothing to wait for.
__global__ __launch_bounds__(kScanThreads) void outlier_scan_kernel(int32_t *__restrict__ indptr, long R) {
    __shared__ int s_wave[kScanThreads / 64];
    int32_t *c = indptr + 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) indptr[0] = 0;
    int carry = 0;
    for (long base = 0; base < R; base += kScanChunk) {
        const long i0 = base + (long)tid * 4;
        int v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < R ? c[i0 + j] : 0;
        v[1] += v[0];
        v[2] += v[1];
        v[3] += v[2];
        int t = v[3];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(t, off, 64);
            if (lane >= off) t += o;
        }
        if (lane == 63) s_wave[wave] = t;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const int s = s_wave[w];
            before += w < wave ? s : 0;
            total += s;
        }
        const int excl = carry + before + t - v[3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < R) c[i0 + j] = v[j] + excl;
        carry += total;
        __syncthreads();
    }
}

template <int IO>
__global__ __launch_bounds__(kRowWaves * 64) void outlier_compact_kernel(const typename ElemOf<IO>::type *__restrict__ x,
                                                                         const int32_t *__restrict__ indptr,
                                                                         typename ElemOf<IO>::type *__restrict__ data, int32_t *__restrict__ indices,
                                                                         long R, long C, float thr, long max_nnz) {
    using E = typename ElemOf<IO>::type;
    constexpr int VEC = 16 / (int)sizeof(E);
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;
    const long nw = (long)gridDim.x * kRowWaves;
    for (long r = (long)blockIdx.x * kRowWaves + (threadIdx.x >> 6); r < R; r += nw) {
        const long base = indptr[r];
        if (indptr[r + 1] == base || base >= max_nnz) continue;          // wave-uniform: no entry, or all of them behind the cut
        long running = base;
        walk_row<IO>(x + r * C, (E *)nullptr, C, lane, [&](long c0, int n, E(&e)[VEC]) __attribute__((always_inline)) {
            E keep[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) keep[j] = e[j];
            const uint32_t m = split_values<IO, VEC>(e, n, thr);
            if (__ballot(m != 0) == 0ull) return;
            int pre = 0, tot = 0;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {                                  // entries are in lane order, then slot order
                const unsigned long long b = __ballot((m >> j) & 1u);
                pre += __popcll(b & below);
                tot += __popcll(b);
            }
            long pos = running + pre;
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if ((m >> j) & 1u) {
                    if (pos < max_nnz) {
                        data[pos] = keep[j];
                        indices[pos] = (int32_t)(c0 + j);
                    }
                    ++pos;
                }
            }
            running += tot;
        });
    }
    // the padding behind the stored entries
    const long total = indptr[R];
    const long nthreads = (long)gridDim.x * blockDim.x;
    for (long i = (total < max_nnz ? total : max_nnz) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < max_nnz; i += nthreads) {
        data[i] = 0;
        indices[i] = 0;
    }
}

template <int IO>
int launch_filter_outlier(const void *x, void *inlier, void *data, int32_t *indices, int32_t *indptr, long R, long C, float thr, long max_nnz,
                          void *stream) {
    using E = typename ElemOf<IO>::type;
    if (!x || !inlier || !indptr || R < 1 || C < 1 || max_nnz < 0 || (max_nnz > 0 && (!data || !indices))) return QT_ERR_BAD_ARG;
    if (R > 0x7FFFFFFEl || C > 0x7FFFFFFEl || R * C > 0x7FFFFFFEl || max_nnz > R * C) return QT_ERR_BAD_ARG;
    if (((uintptr_t)x | (uintptr_t)inlier | (uintptr_t)data) % sizeof(E) || ((uintptr_t)indices | (uintptr_t)indptr) % 4) return QT_ERR_UNALIGNED;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = grid_for((size_t)R, kRowWaves, 8);
    outlier_split_kernel<IO><<<grid, kRowWaves * 64, 0, st>>>((const E *)x, (E *)inlier, indptr, R, C, thr);
    if (const int rc = qt_launch_status()) return rc;
    outlier_scan_kernel<<<1, kScanThreads, 0, st>>>(indptr, R);
    if (const int rc = qt_launch_status()) return rc;
    outlier_compact_kernel<IO><<<grid, kRowWaves * 64, 0, st>>>((const E *)x, indptr, (E *)data, indices, R, C, thr, max_nnz);
    return qt_launch_status();
}

// ---- spmm_csr ----------------------------------------------------------------------------------------------------------------------------
constexpr int kSpmmThreads = 1024;           // CSR rows one workgroup walks at a time
constexpr int kSpmmCodeMax = 256;
constexpr int kSpmmGroup = 16;             // entries of a row summed on their own before they join the row's sum
constexpr int kSpmmLds = 160 * 1024;         // a workgroup's LDS on gfx950
constexpr int kSpmmTileBytes = kSpmmLds - kSpmmCodeMax * 4 - 16;

struct SpmmArgs {
    const void *data;
    const int32_t *indices, *indptr;
    long cap, M;
    const void *b;
    long N, K;
    const void *scale;           // nullable; [scale_rows][scale_cols], element (i0, i1) of the stored B takes scale[i0 / div0][i1 / div1]
    long scale_cols;
    int div0, div1;
    const void *code;            // nullable; n_code <= 256 values
    int n_code;
    void *y;
    long rows_per_block;
};

// TN values of one tile row, LDS -> registers, with the widest reads the row's size allows
template <int IO, int TN>
__device__ __forceinline__ void read_tile_row(const typename ElemOf<IO>::type *p, float (&b)[TN]) {
    using E = typename ElemOf<IO>::type;
    constexpr int BYTES = TN * (int)sizeof(E);
    E e[TN];
    if constexpr (BYTES % 16 == 0) {
#pragma unroll
        for (int q = 0; q < BYTES / 16; ++q) {
            const uint4 w = ((const uint4 *)p)[q];
            __builtin_memcpy((char *)e + 16 * q, &w, 16);
        }
    } else if constexpr (BYTES == 8) {
        const uint2 w = *(const uint2 *)p;
        __builtin_memcpy(e, &w, 8);
    } else if constexpr (BYTES == 4) {
        const uint32_t w = *(const uint32_t *)p;
        __builtin_memcpy(e, &w, 4);
    } else {
        e[0] = p[0];
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) b[j] = elem_f<IO>(e[j]);
}

// KN: B is stored [K][N] (weight_transposed), else [N][K].
template <int IO, int TN, bool KN>
__global__ __launch_bounds__(kSpmmThreads) void spmm_csr_kernel(const SpmmArgs a) {
    using E = typename ElemOf<IO>::type;
    extern __shared__ uint4 s_raw[];
    E *tile = (E *)s_raw;                                             // [K][TN]
    float *s_code = (float *)((char *)s_raw + (((size_t)a.K * TN * sizeof(E) + 15) & ~(size_t)15));
    const int tid = threadIdx.x;
    const long n0 = (long)blockIdx.x * TN;
    const E *B = (const E *)a.b, *scale = (const E *)a.scale;
    const long K = a.K, N = a.N;

    if (a.code) {
        for (int i = tid; i < a.n_code; i += kSpmmThreads) s_code[i] = elem_f<IO>(((const E *)a.code)[i]);
        __syncthreads();
    }
    // Bd of element (i0, i1) of the stored B: the composite's B_code[B.long()] * expand(scale), in the tensor's dtype
    auto operand = [&](long i0, long i1) __attribute__((always_inline)) -> E {
        E raw = B[i0 * (KN ? N : K) + i1];
        if (a.code) {
            const float v = elem_f<IO>(raw);
            int ci = __builtin_fabsf(v) < 65536.0f ? (int)v : a.n_code;      // a NaN or a huge value is no index
            ci += ci < 0 ? a.n_code : 0;                                     // torch's negative indices
            raw = elem_of<IO>((unsigned)ci < (unsigned)a.n_code ? s_code[ci] : 0.0f);
        }
        if (scale) raw = elem_of<IO>(elem_f<IO>(raw) * elem_f<IO>(scale[(i0 / a.div0) * a.scale_cols + i1 / a.div1]));
        return raw;
    };
    if constexpr (KN) {
        for (long f = tid; f < K * TN; f += kSpmmThreads) {
            const long k = f / TN;
            const int j = (int)(f % TN);
            tile[f] = n0 + j < N ? operand(k, n0 + j) : (E)0;
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < TN; ++j) {
            const bool live = n0 + j < N;
            for (long k = tid; k < K; k += kSpmmThreads) tile[k * TN + j] = live ? operand(n0 + j, k) : (E)0;
        }
    }
    __syncthreads();

    const E *data = (const E *)a.data;
    const long rbeg = (long)blockIdx.y * a.rows_per_block;
    const long rend = rbeg + a.rows_per_block < a.M ? rbeg + a.rows_per_block : a.M;
    constexpr int VW = TN * (int)sizeof(E) >= 16 ? 16 / (int)sizeof(E) : TN;     // elements per output store
    const bool vec_store = VW > 1 && N % VW == 0 && ((uintptr_t)a.y % (VW * sizeof(E))) == 0;
    for (long r = rbeg + tid; r < rend; r += kSpmmThreads) {
        // a truncated CSR counts entries it does not hold: nothing at or behind `cap` is read
        long s = a.indptr[r], e = a.indptr[r + 1];
        s = s < 0 ? 0 : (s > a.cap ? a.cap : s);
        e = e < s ? s : (e > a.cap ? a.cap : e);
        // groups of kSpmmGroup entries are summed on their own and the group sums added in order: the rounding error of a long row
        // grows with (group + row / group) roundings instead of the row's length
        float acc[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = 0.0f;
        for (long i0 = s; i0 < e; i0 += kSpmmGroup) {
            const long i1 = i0 + kSpmmGroup < e ? i0 + kSpmmGroup : e;
            float part[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) part[j] = 0.0f;
            for (long i = i0; i < i1; ++i) {
                const int32_t idx = a.indices[i];
                const float v = elem_f<IO>(data[i]);
                if ((unsigned long)idx < (unsigned long)K) {                  // an index outside [0, K) is skipped
                    float b[TN];
                    read_tile_row<IO, TN>(tile + (long)idx * TN, b);
#pragma unroll
                    for (int j = 0; j < TN; ++j) part[j] = __builtin_fmaf(v, b[j], part[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] += part[j];
        }
        E *yr = (E *)a.y + r * N + n0;
        E o[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) o[j] = elem_of<IO>(acc[j]);
        if (vec_store) {
#pragma unroll
            for (int j = 0; j < TN; j += VW) {
                if (n0 + j < N) {
                    if constexpr (VW * sizeof(E) == 16) {
                        uint4 w;
                        __builtin_memcpy(&w, &o[j], 16);
                        *(uint4 *)(yr + j) = w;
                    } else if constexpr (VW * sizeof(E) == 8) {
                        uint2 w;
                        __builtin_memcpy(&w, &o[j], 8);
                        *(uint2 *)(yr + j) = w;
                    } else {
                        uint32_t w;
                        __builtin_memcpy(&w, &o[j], 4);
                        *(uint32_t *)(yr + j) = w;
                    }
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (n0 + j < N) yr[j] = o[j];
        }
    }
}

template <int IO, int TN, bool KN>
int launch_spmm_tile(const SpmmArgs &args, hipStream_t st) {
    using E = typename ElemOf<IO>::type;
    if (const int rc = qt_allow_lds<spmm_csr_kernel<IO, TN, KN>>(kSpmmLds)) return rc;
    SpmmArgs a = args;
    const long tiles = (a.N + TN - 1) / TN;
    const long chunks = (a.M + kSpmmThreads - 1) / kSpmmThreads;
    long by = (qt_cu_count() + tiles - 1) / tiles;                      // few feature tiles: split the rows so that every CU has work
    by = by < 1 ? 1 : (by > chunks ? chunks : by);
    by = by > 65535 ? 65535 : by;
    a.rows_per_block = (a.M + by - 1) / by;
    const size_t lds = (((size_t)a.K * TN * sizeof(E) + 15) & ~(size_t)15) + kSpmmCodeMax * 4;
    spmm_csr_kernel<IO, TN, KN><<<dim3((unsigned)tiles, (unsigned)by), kSpmmThreads, lds, st>>>(a);
    return qt_launch_status();
}

template <int IO, bool KN>
int launch_spmm_layout(const SpmmArgs &a, hipStream_t st) {
    using E = typename ElemOf<IO>::type;
    int tn = 16;                                                        // the widest tile whose TN rows of the operand fit in LDS
    while (tn > 1 && ((size_t)a.K * tn * sizeof(E) > (size_t)kSpmmTileBytes || tn / 2 >= a.N)) tn >>= 1;
    if ((size_t)a.K * tn * sizeof(E) > (size_t)kSpmmTileBytes) return QT_ERR_BAD_ARG;
    switch (tn) {
    case 16: return launch_spmm_tile<IO, 16, KN>(a, st);
    case 8: return launch_spmm_tile<IO, 8, KN>(a, st);
    case 4: return launch_spmm_tile<IO, 4, KN>(a, st);
    case 2: return launch_spmm_tile<IO, 2, KN>(a, st);
    default: return launch_spmm_tile<IO, 1, KN>(a, st);
    }
}

template <int IO>
int launch_spmm_csr(const void *data, const int32_t *indices, const int32_t *indptr, long cap, long M, const void *b, long N, long K, int b_is_kn,
                    const void *scale, long scale_rows, long scale_cols, int div0, int div1, const void *code, int n_code, void *y, void *stream) {
    using E = typename ElemOf<IO>::type;
    if (M < 0 || N < 0 || cap < 0) return QT_ERR_BAD_ARG;
    if (M == 0 || N == 0) return QT_OK;
    if (!indptr || !b || !y || K < 1 || (cap > 0 && (!data || !indices))) return QT_ERR_BAD_ARG;
    if (M > 0x7FFFFFFEl || N > 0x7FFFFFFEl || K > 0x7FFFFFFEl || cap > 0x7FFFFFFEl) return QT_ERR_BAD_ARG;
    if (scale) {                                                        // the scale must cover B: rows (d0 - 1) / div0, columns (d1 - 1) / div1
        if (scale_rows < 1 || scale_cols < 1 || div0 < 1 || div1 < 1) return QT_ERR_BAD_ARG;
        const long d0 = b_is_kn ? K : N, d1 = b_is_kn ? N : K;
        if ((d0 - 1) / div0 >= scale_rows || (d1 - 1) / div1 >= scale_cols) return QT_ERR_BAD_ARG;
    }
    if (code && (n_code < 1 || n_code > kSpmmCodeMax)) return QT_ERR_BAD_ARG;
    if (((uintptr_t)data | (uintptr_t)b | (uintptr_t)scale | (uintptr_t)code | (uintptr_t)y) % sizeof(E) ||
        ((uintptr_t)indices | (uintptr_t)indptr) % 4)
        return QT_ERR_UNALIGNED;
    const SpmmArgs a{data, indices, indptr, cap, M, b, N, K, scale, scale_cols, div0, div1, code, code ? n_code : 0, y, 0};
    return b_is_kn ? launch_spmm_layout<IO, true>(a, (hipStream_t)stream) : launch_spmm_layout<IO, false>(a, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int qt_filter_outlier_bf16(const uint16_t *x_dev, uint16_t *inlier_dev, uint16_t *data_dev, int32_t *indices_dev, int32_t *indptr_dev, long rows,
                           long cols, float threshold, long max_nnz, void *stream) {
    return launch_filter_outlier<kIoBf16>(x_dev, inlier_dev, data_dev, indices_dev, indptr_dev, rows, cols, threshold, max_nnz, stream);
}
int qt_filter_outlier_f32(const float *x_dev, float *inlier_dev, float *data_dev, int32_t *indices_dev, int32_t *indptr_dev, long rows, long cols,
                          float threshold, long max_nnz, void *stream) {
    return launch_filter_outlier<kIoF32>(x_dev, inlier_dev, data_dev, indices_dev, indptr_dev, rows, cols, threshold, max_nnz, stream);
}

int qt_spmm_csr_bf16(const uint16_t *data_dev, const int32_t *indices_dev, const int32_t *indptr_dev, long capacity, long rows, const uint16_t *b_dev,
                     long N, long K, int b_is_kn, const uint16_t *scale_dev, long scale_rows, long scale_cols, int scale_div0, int scale_div1,
                     const uint16_t *code_dev, int n_code, uint16_t *y_dev, void *stream) {
    return launch_spmm_csr<kIoBf16>(data_dev, indices_dev, indptr_dev, capacity, rows, b_dev, N, K, b_is_kn, scale_dev, scale_rows, scale_cols, scale_div0,
                                    scale_div1, code_dev, n_code, y_dev, stream);
}
int qt_spmm_csr_f32(const float *data_dev, const int32_t *indices_dev, const int32_t *indptr_dev, long capacity, long rows, const float *b_dev, long N,
                    long K, int b_is_kn, const float *scale_dev, long scale_rows, long scale_cols, int scale_div0, int scale_div1, const float *code_dev,
                    int n_code,
                    float *y_dev, void *stream) {
    return launch_spmm_csr<kIoF32>(data_dev, indices_dev, indptr_dev, capacity, rows, b_dev, N, K, b_is_kn, scale_dev, scale_rows, scale_cols, scale_div0,
                                   scale_div1, code_dev, n_code, y_dev, stream);
}

}  // extern "C"
