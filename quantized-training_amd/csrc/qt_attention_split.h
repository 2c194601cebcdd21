// qt_attention_split.h -- what the two split-key attention kernels share: attention_fp8_split_kernel (qt_attention_fp8.hip, FP8
// operands) and attention_rows_split_kernel (qt_attention_rows.hip, bf16 operands).  In both a workgroup = 8 waves takes 64 query rows;
// wave w = 4 grp + wq owns rows 16 wq .. 16 wq + 15, its group grp the keys 64 grp .. 64 grp + 63 of every 128-key block, and lane
// (r, g) holds query row 16 wq + r against keys 16 t + 4 g + {0..3} of each 16-key tile t.
#pragma once
#include "qt_device.h"

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kBlock = 128, kMaxBlocks = 8;                                    // a key block; the strip holds at most 8 of them

// extents: nlive = key blocks holding an unmasked column of one of the 64 rows; wmax / wmin = the largest / smallest extent among
// this wave's 16 rows; my_live = this lane's row (0: a fully masked row, which attends to every key alike)
template <class A>
__device__ __forceinline__ void split_row_extents(const A &a, int b, int h, int q0, int qc, int l, int nkb, int &nlive, int &wmax, int &wmin,
                                                  int &my_live) {
    nlive = nkb, wmax = a.Sk, wmin = a.Sk, my_live = a.Sk;
    if (a.row_live) {
        const int qq = min(q0 + l, a.Sq - 1);
        int lv = a.row_live[b * a.lsb + h * a.lsh + qq * a.lsq];
        my_live = a.row_live[b * a.lsb + h * a.lsh + qc * a.lsq];
        if (lv <= 0) lv = a.Sk;
        int hi = my_live <= 0 ? a.Sk : my_live, lo = max(my_live, 0);       // a fully masked row is walked to the end and masked from column 0
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) lv = max(lv, __shfl_xor(lv, off, 64));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            hi = max(hi, __shfl_xor(hi, off, 64));
            lo = min(lo, __shfl_xor(lo, off, 64));
        }
        nlive = __builtin_amdgcn_readfirstlane(min(nkb, (lv + kBlock - 1) / kBlock));
        wmax = __builtin_amdgcn_readfirstlane(hi);
        wmin = __builtin_amdgcn_readfirstlane(lo);
    }
}

// After sweep 2: the two partial P.V sums meet in LDS.  Group 1 parks its accumulators ([64 rows][D d] fp32 in the block buffers at lds,
// rows padded by 4 floats, which spreads the 16 rows of a store over the banks), then group 0 reads them back with split_partial_sums.
template <int KDT>
__device__ __forceinline__ void split_park_partials(uint8_t *lds, const v4f (&acc)[KDT], int grp, int prow, int g) {
    __syncthreads();
    float *part = (float *)lds;
    if (grp == 1) {
#pragma unroll
        for (int dt = 0; dt < KDT; ++dt) *(float4 *)(part + prow * (16 * KDT + 4) + dt * 16 + 4 * g) = float4{acc[dt][0], acc[dt][1], acc[dt][2], acc[dt][3]};
    }
    __syncthreads();
}
template <int KDT>
__device__ __forceinline__ float4 split_partial_sums(const uint8_t *lds, int prow, int dt, int g) {
    return *(const float4 *)((const float *)lds + prow * (16 * KDT + 4) + dt * 16 + 4 * g);
}

}  // namespace
