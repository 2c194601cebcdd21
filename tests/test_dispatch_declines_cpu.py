"""What the C ABI's entry points answer to a format they have no kernel for: QT_ERR_BAD_DTYPE (-1) from the chain, LayerNorm-train,
softmax-backward, fan-in and attention-train families, QT_ERR_BAD_ARG (-2) from the elementwise passes and the softmax forward.  The
Python routes branch on that split (_native.declined(code, dtype=...)), so it is pinned here per entry point.

Every decline below is answered before the entry point's first HIP call: nothing is launched, no device is needed, and the pointers are
16-byte-aligned host addresses standing in for device memory.  Left out because a device query comes first: qt_attention_fq_bf16 and
its siblings, qt_fake_quant_mx_*, qt_fake_quant_rows_bf16 (their grid is sized by the CU count before the format is looked at);
qt_quantize_mx_* hands the kind to its kernel at run time and has no such decline."""
import ctypes

import pytest

from quantized_training import _native
from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_BAD_DTYPE, QtChainStage, QtFaninItem, QtFormat

_BUF = ctypes.create_string_buffer(4096 + 64)
P = (ctypes.addressof(_BUF) + 63) & ~63              # stands in for every device pointer
assert P % 16 == 0

LUT, IDENTITY, FP_SAT, INT = 0, 1, 2, 3

# formats no rows-only family takes, then those no family takes
KIND_9 = ("kind 9", QtFormat(9, 0, 0, 0.0, 0.0), P)
KIND_5 = ("kind 5", QtFormat(5, 0, 0, 0.0, 0.0), P)           # csrc's kFmtRows is no kind of the ABI
IDENT = ("identity", QtFormat(IDENTITY, 0, 0, 0.0, 0.0), P)
LUT_NO_ROWS = ("table without the row bit", QtFormat(LUT, 0, 0, 0.0, 0.0), P)
LUT_ROWS_NULL = ("row form, NULL table", QtFormat(LUT, 0, 1, 0.0, 0.0), None)
LUT_NULL = ("table, NULL table", QtFormat(LUT, 0, 0, 0.0, 0.0), None)
ROWS_ONLY = [KIND_9, KIND_5, IDENT, LUT_NO_ROWS, LUT_ROWS_NULL]
ANY_KIND = [KIND_9, KIND_5, LUT_NULL]


def _stages(n):
    st = (QtChainStage * n)()
    for s in st:
        s.scale_f32_dev, s.amax_bits_dev, s.out_dev, s.src = P, P, P, -1
    return st


def _fanin(L, fmt, lut):
    items = (QtFaninItem * 1)()
    items[0].x_dev, items[0].fq, items[0].scale_f32_dev, items[0].amax_bits_dev, items[0].out_dev = P, 1, P, P, P
    return L.qt_grad_fanin_bf16(P, items, 1, P, 8, fmt, lut, None)


def _attn_train_bwd(L, fmt, lut):
    return L.qt_attention_train_backward_bf16(P, P, P, P, 64 * 32, 64, 64, P, P, _stages(2), P, P, P, P, None, None, 0.0, None, 0, None, 1.0, 1, 1, 32,
                                              64, 1.0, fmt, lut, None)


# name -> (call(L, fmt, lut), formats it declines, the code)
CALLS = {
    "qt_grad_fanin_bf16": (_fanin, ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_fake_quant_chain_bf16": (lambda L, f, t: L.qt_fake_quant_chain_bf16(P, 1, 8, _stages(1), 1, f, t, -1, 0.0, None, None, 0, None), ROWS_ONLY,
                                 QT_ERR_BAD_DTYPE),
    "qt_gelu_chain_bf16": (lambda L, f, t: L.qt_gelu_chain_bf16(P, P, 1, 8, _stages(2), 2, f, t, None), ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_gelu_backward_chain_bf16": (lambda L, f, t: L.qt_gelu_backward_chain_bf16(P, P, P, 1, 8, _stages(4), 4, f, t, -1, 0.0, None, None, 0, None),
                                    ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_layernorm_train_bf16": (lambda L, f, t: L.qt_layernorm_train_bf16(P, P, P, P, P, P, 1, 8, 1e-5, _stages(1), 1, f, t, None, None, None),
                                ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_layernorm_train_backward_bf16": (lambda L, f, t: L.qt_layernorm_train_backward_bf16(P, P, P, P, P, P, 1, 8, _stages(3), 3, f, t, -1, P, 4096, P, P,
                                                                                          None, None, 0, None), ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_softmax_backward_chain_bf16": (lambda L, f, t: L.qt_softmax_backward_chain_bf16(P, P, P, 1, 8, 1.0, _stages(2), 2, f, t, None), ROWS_ONLY,
                                       QT_ERR_BAD_DTYPE),
    "qt_attention_train_bf16": (lambda L, f, t: L.qt_attention_train_bf16(P, P, P, 64 * 32, 64, 64, None, 0, 0, 0, _stages(5), P, P, None, 1.0, 1, 1, 32, 64,
                                                                          1.0, f, t, None), ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_attention_train_backward_bf16": (_attn_train_bwd, ROWS_ONLY, QT_ERR_BAD_DTYPE),
    "qt_fake_quant_multi_bf16": (lambda L, f, t: L.qt_fake_quant_multi_bf16(P, 1, 1, f, t, None), ROWS_ONLY, QT_ERR_BAD_ARG),
    "qt_fake_quant_bf16": (lambda L, f, t: L.qt_fake_quant_bf16(P, P, 8, f, t, None, None, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_fake_quant_f32": (lambda L, f, t: L.qt_fake_quant_f32(P, P, 8, f, t, None, None, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_vmap_bf16": (lambda L, f, t: L.qt_vmap_bf16(P, P, 8, f, t, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_fake_quant_pc_bf16": (lambda L, f, t: L.qt_fake_quant_pc_bf16(P, P, 1, 1, 8, f, t, None, None, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_fake_quant_pc_f32": (lambda L, f, t: L.qt_fake_quant_pc_f32(P, P, 1, 1, 8, f, t, None, None, None), ANY_KIND, QT_ERR_BAD_ARG),
    # observe only (y NULL, amax given): the vectorised per-channel kernels evaluate the rounder before they look at y, so a table format
    # needs its table here too
    "qt_fake_quant_pc_bf16, observe only": (lambda L, f, t: L.qt_fake_quant_pc_bf16(P, None, 1, 1, 8, f, t, None, P, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_fake_quant_pc_f32, observe only": (lambda L, f, t: L.qt_fake_quant_pc_f32(P, None, 1, 1, 8, f, t, None, P, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_softmax_fq_bf16": (lambda L, f, t: L.qt_softmax_fq_bf16(P, None, P, 1, 1, 1, 8, 0, 0, 0, 1.0, f, t, None, None, None), ANY_KIND, QT_ERR_BAD_ARG),
    "qt_softmax_fq_probs_bf16": (lambda L, f, t: L.qt_softmax_fq_probs_bf16(P, None, P, P, 1, 1, 1, 8, 0, 0, 0, 1.0, f, t, None, None, None), ANY_KIND,
                                 QT_ERR_BAD_ARG),
    # the FP8-code producers take E4M3 / E5M2 only
    "qt_fake_quant_bf16_fp8": (lambda L, f, t: L.qt_fake_quant_bf16_fp8(P, P, P, 16, f, None, None, None), [KIND_9, IDENT, LUT_NO_ROWS], QT_ERR_BAD_ARG),
    "qt_fake_quant_multi_bf16_fp8": (lambda L, f, t: L.qt_fake_quant_multi_bf16_fp8(P, 1, 1, f, None), [KIND_9, IDENT, LUT_NO_ROWS], QT_ERR_BAD_ARG),
}
CASES = [pytest.param(name, fmt, lut, code, id=f"{name}-{label}") for name, (_, fmts, code) in CALLS.items() for label, fmt, lut in fmts]


@pytest.mark.parametrize("name,fmt,lut,code", CASES)
def test_unsupported_format_declines_with_the_family_s_code(name, fmt, lut, code):
    assert CALLS[name][0](_native.lib(), ctypes.byref(fmt), lut) == code


# the ten element-format pairs of csrc/qt_mx_tile.h (QT_MX_E4M3 0, E5M2 1, E2M3 2, E3M2 3, E2M1 4)
MX_PAIRS = {(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (2, 4), (3, 4)}


@pytest.mark.parametrize("fa,fb", [(a, b) for a in range(5) for b in range(5) if (a, b) not in MX_PAIRS])
def test_mx_gemm_declines_a_pair_without_a_kernel(fa, fb):
    # K = 64: 16-byte rows of codes at 4, 6 and 8 bits per element
    assert _native.lib().qt_mx_gemm(P, P, fa, P, P, fb, P, 0, None, 1, 1, 1, 64, 0, 0, None) == QT_ERR_BAD_DTYPE
