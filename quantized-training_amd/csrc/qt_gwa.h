// qt_gwa.h -- the element arithmetic of group-wise affine dequantization, shared by quantized_ops::dequantize's block kernel
// (qt_groupwise.hip) and by the packed-weight kernels (qt_gwa_gemm.hip): one definition, so the two cannot drift apart.
#pragma once
#include "qt_device.h"

namespace {

template <int IO>
__device__ __forceinline__ float rd_io(float f) {            // the result of one torch op in the tensor's dtype
    if constexpr (IO == kIoBf16) return bf16_round(f);
    else return f;
}

// (q - z) * s as two torch ops in the tensor's dtype (decomposed.py:196): both roundings are kept, zero points are not integers
template <int IO>
__device__ __forceinline__ float gwa_dequant(float q, float z, float s) {
    return rd_io<IO>(rd_io<IO>(q - z) * s);
}

}  // namespace
