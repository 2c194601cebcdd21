// qt_splitk.h -- the split-K hand-over between workgroups, shared by linear_fqt_kernel (qt_linear_fqt.hip), conv2d_wgrad_kernel
// (qt_conv_backward.hip), linear_gwa_tall_kernel (qt_gwa_tall.hip) and the SPLIT instantiations of mx_conv_kernel (qt_mx_conv.hip).
//
// S workgroups share an output tile, each over its own part of the contraction.  Nobody ever waits for another workgroup:
//   1. every split stores its partial sums into its slab of the caller's workspace, write-through (store16_sc1);
//   2. every wave drains its stores and the workgroup meets at a barrier; ONE lane then draws the tile's ticket (splitk_draw);
//   3. a workgroup that did not draw the last ticket is done.  The one that did owns the tile: it resets the ticket -- tickets are zero
//      between launches -- and drops what its L2 may still hold of the workspace (splitk_own);
//   4. it reads the partial sums back past its L1 (load16_sc1), adds them IN SPLIT ORDER (splitk_sum) and runs its kernel's epilogue.
// fp32 owners add ALL the partial sums, their own included, starting from zero: no instruction depends on which split arrived last, so
// the bits do not either.  Integer sums are exact in any order, so the int8 convolution starts from the sums in its registers and skips
// its own slab (which is stored all the same: the owner is not known before the ticket is drawn).
//
// Why this is ordered.  The ticket's atomic is RELAXED on purpose: an agent-scope release / acquire pair there would write back and
// invalidate the whole L2, behind up to 20 MB of partial sums.  The ordering is made by hand instead -- valid on gfx942 / gfx950, which
// qt_device.h asserts at compile time:
//   * an sc1 store is written through to memory, and s_waitcnt vmcnt(0) returns only when every store of the wave has been
//     acknowledged there.  Every wave waits, then the barrier: when the one lane issues the atomic, all of the workgroup's partial
//     sums are in memory;
//   * atomics on one address are totally ordered, so the workgroup that reads S - 1 (plus whatever a caller keeps in the upper bits)
//     comes after every other split's atomic, hence after their stores reached memory;
//   * the owner's loads are issued behind the second barrier, carry sc1 (they miss the L1) and, behind the acquire fence, find no
//     line of the workspace in this XCD's L2 that an EARLIER launch left there (the fence invalidates; nothing is written back,
//     and only the owner of a tile pays for it).
//
// Workspace: [tile][split][wave][fragment][64 lanes] of 16 bytes (splitk_slab): a wave's store or load instruction moves one contiguous
// KiB, addressed by a wave-uniform base (an SGPR pair) + a 32-bit lane offset, so no address registers are held per fragment.
#pragma once
#include "qt_device.h"

// what every *_ws entry point asks of the caller's workspace and tickets, in this precedence
inline int qt_splitk_scratch_status(const void *ws, size_t ws_bytes, size_t need_bytes, const void *tickets, size_t n_tickets, size_t need_tickets) {
    if (!ws || !tickets || ws_bytes < need_bytes || n_tickets < need_tickets) return QT_ERR_BAD_ARG;
    if (((uintptr_t)ws & 15u) || ((uintptr_t)tickets & 3u)) return QT_ERR_UNALIGNED;
    return QT_OK;
}

namespace {

// V: any native 16-byte vector (f32x4, v4i).  The compiler pads nothing inside an asm string and knows no hazard of the instruction
// in it.  Two are live here: the base is computed by scalar adds right in front (an SGPR written by the SALU needs wait states before a
// vector memory instruction reads it: s_nop 4 opens the string), and the sums are copied out of the accumulation registers into the
// same four VGPRs for every fragment (a 16-byte store reads its data over several cycles: s_nop 1 ends the string, so that the next
// copy cannot overwrite them).
template <class V>
__device__ __forceinline__ void store16_sc1(const V *sbase, uint32_t voff, V v) {
    static_assert(sizeof(V) == 16, "one global_store_dwordx4");
    asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1\n\ts_nop 1" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
template <class V>
__device__ __forceinline__ V load16_sc1(const V *sbase, uint32_t voff) {
    static_assert(sizeof(V) == 16, "one global_load_dwordx4");
    V v;
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 sc1" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
    return v;
}
__device__ __forceinline__ uint32_t splitk_lane_off() { return (threadIdx.x & 63u) * 16u; }

// the slab of the calling wave in split `split` of tile `tile`: FRAGS fragments of 64 lanes x 16 bytes (WAVES per workgroup)
template <int WAVES, int FRAGS, class V>
__device__ __forceinline__ V *splitk_slab(V *ws, long tile, int nsplit, int split) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return ws + (((tile * nsplit + split) * WAVES + wave) * FRAGS) * 64L;
}

// Publish and draw (step 2): returns to every thread what the tile's ticket held before this workgroup added `inc`.  `word` is any
// 4 bytes of LDS the workgroup no longer needs (the first barrier also says: every wave is done with whatever lay there).
__device__ __forceinline__ unsigned int splitk_draw(unsigned int *ticket, unsigned int inc, volatile unsigned int *word) {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) *word = __hip_atomic_fetch_add(ticket, inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *word;
}

// Take ownership (step 3), by the workgroup that drew the last ticket.
__device__ __forceinline__ void splitk_own(unsigned int *ticket) {
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // drop what this XCD's L2 holds of the workspace from earlier launches
}

// The in-order sum (step 4) of the fp32 kernels over a wave's A x B fragments, fragment (i, j) at index i B + j of its slab: acc = the
// partial sums of ALL the splits q = 0 .. nsplit - 1 in that order, from ZERO (what acc holds is ignored).  A rolled loop with one
// split's fragments live and one wait per split.  (The int8 convolution, which adds onto the sums in its AGPRs and leaves its own
// split out, writes the same loop in its kernel: through this function hipcc moved its 64 sums into VGPRs for the whole loop and
// copied them once per split, 0.25 us per launch.)
template <int WAVES, int A, int B, class V>
__device__ __forceinline__ void splitk_sum(V (&acc)[A][B], const V *ws, long tile, int nsplit) {
    const V *const base = splitk_slab<WAVES, A * B>(ws, tile, nsplit, 0);
    const uint32_t voff = splitk_lane_off();
#pragma unroll
    for (int i = 0; i < A; ++i)
#pragma unroll
        for (int j = 0; j < B; ++j) acc[i][j] = V{};
#pragma unroll 1
    for (int q = 0; q < nsplit; ++q) {
        V part[A][B];
#pragma unroll
        for (int i = 0; i < A; ++i)
#pragma unroll
            for (int j = 0; j < B; ++j) part[i][j] = load16_sc1(base + (long)q * WAVES * A * B * 64 + (i * B + j) * 64, voff);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < A; ++i)
#pragma unroll
            for (int j = 0; j < B; ++j) {
                asm volatile("" : "+v"(part[i][j]));
                acc[i][j] += part[i][j];
            }
    }
}

}  // namespace
