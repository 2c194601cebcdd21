// qt_qdq.h -- one element of quantized_ops::quantize / dequantize (decomposed.py:166-262) and its narrowing to an int8 code, shared by
// the elementwise kernels (qt_elementwise.hip: qt_quantize_*, qt_dequantize_*, qt_quantize_codes_nhwc_*) and by the convolution
// epilogues that write the next layer's codes (qt_mx_tile.h: emit_codes_tile behind qt_q8_*_codes): one definition, so the two cannot drift apart.
#pragma once
#include "qt_device.h"

namespace {

struct QdqArgs {
    const uint16_t *in_lut;    // applied first (dequantize's input_qmap) or NULL
    const uint16_t *out_lut;   // applied last (quantize's qmap / dequantize's output_qmap) or NULL
    qt_format out_fmt;         // closed form for out_lut when kind != LUT and out_lut == NULL
    int use_out;               // 1 = apply out rounding
    int mode;                  // 0 = x / s [+ zp], 1 = (x [- zp]) * s
};

// one element of quantize / dequantize: value `v` is kept in the tensor dtype after every op (bf16 ops round to bf16)
template <int IO>
__device__ __forceinline__ float qdq_value(float v, const QdqArgs &a, float s, float z, bool has_zp) {
    auto round_io = [](float f) -> float {
        if constexpr (IO == kIoBf16) return qt_u2f(pack_bf16x2(f, 0.0f) << 16);
        else return f;
    };
    auto lookup = [&](const uint16_t *t, float f) -> float {
        uint32_t img = (IO == kIoBf16) ? qt_f2u(f) : qt_fold_img(qt_f2u(f));
        return qt_bf2f(t[img >> 16]);
    };
    if (a.in_lut) v = lookup(a.in_lut, v);
    if (a.mode == 0) {
        v = round_io(v / s);
        if (has_zp) v = round_io(v + z);
    } else {
        if (has_zp) v = round_io(v - z);
        v = round_io(v * s);
    }
    if (a.use_out) {
        if (a.out_lut) v = lookup(a.out_lut, v);
        else {
            uint32_t img = (IO == kIoBf16) ? qt_f2u(v) : qt_fold_img(qt_f2u(v));
            v = qt_u2f(qt_apply_format_img(a.out_fmt, img));
        }
    }
    return v;
}

// code = narrow(qdq_value(x)) with the quantize arguments (mode 0, no zero point, the map from global memory): the value the
// quantize kernel would store, narrowed as torch's .to(int8) narrows an integer in [-128, 127].  Anything else a map could
// hold: truncated toward zero, saturated to [-128, 127], NaN -> 0.
__device__ __forceinline__ uint32_t code_of(float v) {
    if (v != v) return 0u;
    v = fminf(fmaxf(v, -128.0f), 127.0f);
    return (uint32_t)(int)v & 0xFFu;
}

}  // namespace
