// qt_histogram.hip -- record_histogram on a device tensor as ONE launch that reads x once.
//
// The reference (fake_quantize.py:348-350) runs  exp = floor(log2(|float(x)|));  histogram += histc(exp, 254, -126, 127)  -- six
// launches and ~38 B of traffic per bf16 element.  Here: 2 B per element, the closed form and the counting scheme of qt_histogram.h.
//
// Contract, per call and per bin b:  hist[b] = fl32(hist[b] + fl32(c_b))  with c_b the EXACT integer count of the call.  That is what
// the composite computes whenever its own per-call count is exact, i.e. while no bin receives more than 2^24 elements in one call;
// beyond that histc's fp32 counting saturates or depends on the order of its device atomics, and the exact count here is the
// definition.  Counts are u32, so n >= 2^32 is refused.
//
// Loads: 16 bytes per lane, a scalar head up to the first 16-byte boundary and a scalar tail, so any 2-byte aligned base and any n
// are served.  1024-thread workgroups (one 32 KiB replica table each), two loads in flight per lane, at most two workgroups per
// compute unit with a grid-stride loop: every workgroup ends in up to 254 agent-scope atomics on ONE kilobyte, so there are few.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_device.h"
#include "qt_histogram.h"

namespace {

constexpr int kBlock = 1024, kInFlight = 2, kBlocksPerCu = 2;

template <bool F16>
__global__ __launch_bounds__(kBlock) void exp_histogram_kernel(const uint16_t *__restrict__ x, size_t n, size_t head, size_t nvec,
                                                              HistArgs h) {
    __shared__ uint32_t s_hist[kHistWords];
    hist_lds_zero<kBlock>(s_hist);
    __syncthreads();
    const uint4 *xv = (const uint4 *)(x + head);
    constexpr size_t kTile = (size_t)kBlock * kInFlight;
    const size_t nfull = nvec / kTile;
    for (size_t t = blockIdx.x; t < nfull; t += gridDim.x) {
        const size_t base = t * kTile + threadIdx.x;
        uint4 v[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) v[u] = xv[base + (size_t)u * kBlock];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) hist_add_vec<F16>(s_hist, v[u]);
    }
    // ragged last tile: the block that would own it in the grid-stride order
    if (nfull % gridDim.x == blockIdx.x)
        for (size_t i = nfull * kTile + threadIdx.x; i < nvec; i += kBlock) hist_add_vec<F16>(s_hist, xv[i]);
    if (blockIdx.x == 0 && threadIdx.x < head) hist_add_elem<F16>(s_hist, x[threadIdx.x]);                 // head < 8
    if (blockIdx.x == gridDim.x - 1)
        for (size_t i = head + nvec * 8 + threadIdx.x; i < n; i += kBlock) hist_add_elem<F16>(s_hist, x[i]);
    hist_commit<kBlock>(s_hist, h);
}

template <bool F16>
int launch_exp_histogram(const uint16_t *x, size_t n, float *hist, uint32_t *counts, uint32_t *ticket, void *stream) {
    if (n == 0) return QT_OK;
    if (!x || !hist || !counts || !ticket || n > 0xFFFFFFFFull) return QT_ERR_BAD_ARG;
    if (((uintptr_t)x & 1u) || (((uintptr_t)hist | (uintptr_t)counts | (uintptr_t)ticket) & 3u)) return QT_ERR_UNALIGNED;
    size_t head = ((16u - ((uintptr_t)x & 15u)) & 15u) / 2;
    if (head > n) head = n;
    const size_t nvec = (n - head) / 8;
    const unsigned grid = grid_for(nvec, (size_t)kBlock * kInFlight, kBlocksPerCu);
    exp_histogram_kernel<F16><<<grid, kBlock, 0, (hipStream_t)stream>>>(x, n, head, nvec, HistArgs{hist, counts, ticket});
    return qt_launch_status();
}

}  // namespace

extern "C" {

int qt_exp_histogram_bf16(const uint16_t *x_dev, size_t n, float *hist_f32_dev, uint32_t *counts_u32_dev, uint32_t *ticket_dev,
                          void *stream) {
    return launch_exp_histogram<false>(x_dev, n, hist_f32_dev, counts_u32_dev, ticket_dev, stream);
}
int qt_exp_histogram_f16(const uint16_t *x_dev, size_t n, float *hist_f32_dev, uint32_t *counts_u32_dev, uint32_t *ticket_dev,
                         void *stream) {
    return launch_exp_histogram<true>(x_dev, n, hist_f32_dev, counts_u32_dev, ticket_dev, stream);
}
int qt_exp_histogram_plan(size_t *tile_elems, size_t *max_workgroups) {
    if (tile_elems) *tile_elems = (size_t)kBlock * kInFlight * 8;
    if (max_workgroups) *max_workgroups = (size_t)qt_cu_count() * kBlocksPerCu;
    return QT_OK;
}

}  // extern "C"
