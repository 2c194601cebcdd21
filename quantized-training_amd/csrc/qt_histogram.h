// qt_histogram.h -- the exponent histogram's device pieces, shared by its own launch (qt_histogram.hip) and by the fake-quant pass
// that takes it on the way (qt_elementwise.hip, fq_kernel<..., HIST = true>).
//
// What is counted (fake_quantize.py:348-350 upstream: histc(floor(log2 |float(x)|), 254, -126, 127)): for a bf16 or fp16 element,
// converted exactly to fp32, the bin is the fp32 exponent field E = (bits >> 23) & 0xFF: 1 <= E <= 254 counts into bin E - 1; E = 0
// (zeros and what is subnormal AS fp32) and E = 255 (inf, NaN) count nowhere, as histc leaves them out.  Checked by enumeration of
// all 65 536 patterns of both types (tests/test_histogram_cpu.py).  NOT valid for fp32 inputs: floor(log2f(x)) rounds up for most
// values one ulp below a power of two, so fp32 tensors stay with the torch composite.
//
// Inside a workgroup: 256 rows (one per E; rows 0 and 255 take what counts nowhere, so no lane is ever masked off) x 32 replicas,
// word [E][lane & 31] -- 32 KiB.  A ds_add_u32 is serviced in lane groups {0-31}, {32-63}; bank = word index mod 32 = lane & 31, so
// the 32 lanes of a group hit 32 banks whatever their bins are (all-equal data included), and lanes l / l + 32 are never in one group.
// Across workgroups: the non-zero rows are added to counts[256] with relaxed agent-scope u32 atomics, then one lane draws a ticket;
// whoever draws the last one takes every count back with an atomic exchange against zero (performed where the adds were, so never
// served by its L1 or its XCD's L2), adds it to hist ONCE per bin -- hist[b] = fl32(hist[b] + fl32(c_b)), c_b exact -- and zeroes
// the ticket.  Nobody waits; integer sums do not depend on arrival order, so every run gives the same bits.  No float atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_device.h"

namespace {

constexpr int kHistRows = 256, kHistReplicas = 32, kHistWords = kHistRows * kHistReplicas;   // 32 KiB of LDS
constexpr int kHistBins = 254;

struct HistArgs {
    float *hist;             // [254] fp32
    uint32_t *counts;        // [256] zero between launches (the last workgroup leaves it so)
    uint32_t *ticket;        // [1] likewise
};

// (the barrier that publishes the zeros is the caller's)
template <int BLOCK>
__device__ __forceinline__ void hist_lds_zero(uint32_t *s) {
    for (int i = threadIdx.x; i < kHistWords / 4; i += BLOCK) ((uint4 *)s)[i] = uint4{0u, 0u, 0u, 0u};
}

// one element whose fp32 exponent field is E (0..255)
__device__ __forceinline__ void hist_add(uint32_t *s, uint32_t E) {
    __hip_atomic_fetch_add(s + ((E << 5) | (threadIdx.x & 31u)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// two bf16 elements in one word: the exponent field of bf16 IS the fp32 one
__device__ __forceinline__ void hist_add_bf16x2(uint32_t *s, uint32_t w) {
    hist_add(s, (w >> 7) & 0xFFu);
    hist_add(s, (w >> 23) & 0xFFu);
}
// the fp32 exponent field of an fp16 pattern: normals e5 + 112, subnormals m 2^-24 -> 103 + (index of m's top bit), i.e. bins 102..111
__device__ __forceinline__ uint32_t hist_f16_field(uint32_t h) {
    const uint32_t e5 = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    if (e5 == 31u) return 255u;
    if (e5 != 0u) return e5 + 112u;
    return m ? 103u + (31u - (uint32_t)__clz((int)m)) : 0u;
}
template <bool F16>
__device__ __forceinline__ void hist_add_word(uint32_t *s, uint32_t w) {
    if constexpr (F16) {
        hist_add(s, hist_f16_field(w & 0xFFFFu));
        hist_add(s, hist_f16_field(w >> 16));
    } else {
        hist_add_bf16x2(s, w);
    }
}
template <bool F16>
__device__ __forceinline__ void hist_add_vec(uint32_t *s, const uint4 &v) {
    hist_add_word<F16>(s, v.x);
    hist_add_word<F16>(s, v.y);
    hist_add_word<F16>(s, v.z);
    hist_add_word<F16>(s, v.w);
}
template <bool F16>
__device__ __forceinline__ void hist_add_elem(uint32_t *s, uint16_t h) {
    hist_add(s, F16 ? hist_f16_field(h) : (((uint32_t)h >> 7) & 0xFFu));
}

// The workgroup's rows -> counts, the ticket, and (last arriver) counts -> hist.  Every thread of the workgroup calls it, once, after its
// last hist_add.  The "I am last" word goes through s[0] (row 0 counts nowhere and has been read by then): no second LDS object.
template <int BLOCK>
__device__ __forceinline__ void hist_commit(uint32_t *s, const HistArgs &h) {
    __syncthreads();                                             // every wave's LDS adds are in
    for (int r = threadIdx.x; r < kHistRows; r += BLOCK) {
        uint32_t c = 0;
#pragma unroll 8
        for (int k = 0; k < kHistReplicas; ++k) c += s[(r << 5) | ((k + r) & 31)];      // rotated: lane r starts at bank r & 31
        if (c != 0u && r >= 1 && r <= kHistBins) __hip_atomic_fetch_add(h.counts + r, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // this wave's adds have been performed
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // (kept behind the fence, in this order, in front of the ticket)
        s[0] = __hip_atomic_fetch_add(h.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s[0] != gridDim.x - 1u) return;                          // not the last one: done, nobody waits
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int r = threadIdx.x; r < kHistRows; r += BLOCK) {
        if (r < 1 || r > kHistBins) continue;
        const uint32_t c = __hip_atomic_exchange(h.counts + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c != 0u) h.hist[r - 1] = h.hist[r - 1] + (float)c;   // one rounding of the count, one of the sum
    }
    if (threadIdx.x == 0) __hip_atomic_store(h.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
