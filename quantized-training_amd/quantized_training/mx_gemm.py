"""linear_mx / matmul_mx on gfx950's block-scaled matrix instruction (upstream decomposed.py:304-363).

The reference states these ops as "multiply each operand by its expanded block scales, then F.linear /
torch.matmul".  When the element values are one of the formats v_mfma_scale_f32_16x16x128_f8f6f4 takes
(fp8_e4m3, fp8_e5m2, fp6_e2m3, fp6_e3m2, fp4_e2m1) and the block scales are powers of two over blocks of a
multiple of 32 elements, the same product is computed from the element codes and E8M0 scale bytes directly
(qt_mx_pack + qt_mx_gemm in libqt_hip.so): no dequantized copy of either operand is ever written.

The ops only see tensors, so what an operand holds is recovered from
  * the value map it was quantized with (torch.ops.quantized_ops.quantize / quantize_mx remember the format
    on their result -- the record and its readers are mx_operand.py; a map is recognised by its tag or, once per
    buffer, by content);
  * the packer itself, which refuses (flag) values outside the format and scales that are not 2^e; weights are
    packed once and cached on the tensor, so that check costs one host sync per weight, not per call.
Anything else (codebooks, int formats, block size 16, fp8 scales ...) returns None and the caller runs the
reference formulation.  QT_MX_GEMM=0 disables the native path.
"""
import ctypes

import torch

from . import _native, mx_operand, switches
from .fake_quantize import _stream_ptr

__all__ = ["mx_linear_or_none", "mx_matmul_or_none", "STATS"]

# the kernels' facts live with the record (mx_operand.py); tests and tools read them here
FMT_ID, _BITS, _PAIRS = mx_operand.FMT_ID, mx_operand.BITS, mx_operand.PAIRS


class _Stats:
    """How many GEMMs took the native path (tests assert on it; a silent fallback would hide a regression)."""
    def __init__(self):
        self.native = 0
        self.fallback = 0

    def reset(self):
        self.native = self.fallback = 0


STATS = _Stats()
_DEBUG = False            # set mx_gemm._DEBUG = True to print why a problem took the reference formulation


def _fallback(why):
    STATS.fallback += 1
    if _DEBUG:
        print("mx_gemm: reference formulation:", why, flush=True)
    return None


def _enabled():
    return switches.on("QT_MX_GEMM")


def _pack(values, scale, fmt_id, block_size, batch, rows, K, x_strides, s_strides, check):
    """-> (codes [batch, rows, K*bits/8] u8, e8m0 [batch, rows, K/32] u8) or None when the packer refuses."""
    L = _native.lib()
    dev = values.device
    codes = torch.empty((batch, rows, mx_operand.row_bytes(K, fmt_id)), dtype=torch.uint8, device=dev)
    e8 = torch.empty((batch, rows, K // 32), dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
    _native.check(L.qt_mx_pack(values.data_ptr(), scale.data_ptr(), int(values.dtype == torch.float32), codes.data_ptr(),
                               e8.data_ptr(), batch, rows, K, *x_strides, *s_strides, block_size, fmt_id,
                               bad.data_ptr() if check else None, _stream_ptr(values)), "qt_mx_pack")
    if check and int(bad.item()) != 0:
        return None
    return codes, e8


def _pack_rows(w, s, fmt_id, block_size):
    """The packer over contiguous [rows, K] values and [rows, K / bs] scales with its check on: what a constant operand goes through."""
    rows, K = w.shape
    return _pack(w, s, fmt_id, block_size, 1, rows, K, (0, K, 1), (0, s.shape[-1], 1), check=True)


def _weight_operand(weight, scale, block_size):
    """Constant operand [N, K] (+ scale [N, K / bs]): packed once, cached on the tensor object."""
    return mx_operand.weight_operand(weight, scale, block_size, mx_operand.GEMM_SLOT,
                                     lambda: (weight.contiguous(), scale.contiguous()), weight.shape[1], _pack_rows)


def _common_ok(x, scale, code, block_size):
    return (code is None and scale is not None and isinstance(block_size, int) and block_size >= 32 and block_size % 32 == 0
            and x.dtype in (torch.bfloat16, torch.float32) and scale.dtype == x.dtype and x.device.type == "cuda")


def mx_linear_or_none(input, weight, bias, input_scale, weight_scale, block_size, input_code, weight_code):
    if not _enabled() or not _common_ok(input, input_scale, input_code, block_size) \
            or not _common_ok(weight, weight_scale, weight_code, block_size) or weight.dtype != input.dtype:
        return None
    fa, pow2 = mx_operand.format_of(input), mx_operand.is_pow2(input_scale)
    if fa not in FMT_ID or not pow2 or weight.dim() != 2 or input.dim() < 2:
        return _fallback(f"input format {fa}, power-of-two scale {pow2}")
    K = input.shape[-1]
    N = weight.shape[0]
    if weight.shape[1] != K or K % 32 or K % block_size or input.numel() == 0:
        return _fallback(f"K = {K}, block {block_size}")
    wop = _weight_operand(weight, weight_scale, block_size)
    fid = FMT_ID[fa]
    if wop is None or (fid, wop[0]) not in _PAIRS or not mx_operand.row_is_whole_chunks(K, fid):
        return _fallback(f"weight operand {None if wop is None else wop[0]} with input format {fid}, K = {K}")
    x = input.contiguous()
    M = x.numel() // K
    pre = mx_operand.operand(input, mx_operand.ROWS, fid, block_size, M, K)          # quantize_mx already emitted the packed operand
    if pre is None:
        s = input_scale.contiguous()
        pre = _pack(x, s, fid, block_size, 1, M, K, (0, K, 1), (0, s.shape[-1], 1), check=False)
    a_codes, a_e8 = pre
    out = torch.empty(input.shape[:-1] + (N,), dtype=input.dtype, device=input.device)
    b = bias.to(input.dtype).contiguous() if bias is not None else None
    L = _native.lib()
    _native.check(L.qt_mx_gemm(a_codes.data_ptr(), a_e8.data_ptr(), fid, wop[1].data_ptr(), wop[2].data_ptr(), wop[0],
                               out.data_ptr(), int(out.dtype == torch.float32), b.data_ptr() if b is not None else None,
                               1, M, N, K, 0, 0, _stream_ptr(x)), "qt_mx_gemm")
    STATS.native += 1
    return out


def mx_matmul_or_none(a, b, a_scale, b_scale, block_size, a_code, b_code):
    """a [..., M, K] with blocks along K (last axis); b [..., K, N] with blocks along K (axis -2)."""
    if not _enabled() or not _common_ok(a, a_scale, a_code, block_size) or not _common_ok(b, b_scale, b_code, block_size) \
            or a.dtype != b.dtype:
        return None
    fa, fb = mx_operand.format_of(a), mx_operand.format_of(b)
    ok = (fa in FMT_ID and fb in FMT_ID and mx_operand.is_pow2(a_scale) and mx_operand.is_pow2(b_scale)
          and a.dim() >= 2 and b.dim() >= 2 and a.shape[:-2] == b.shape[:-2] and a.shape[-1] == b.shape[-2])
    if ok:
        M, K = a.shape[-2:]
        N = b.shape[-1]
        fia, fib = FMT_ID[fa], FMT_ID[fb]
        ok = ((fia, fib) in _PAIRS and K % 32 == 0 and K % block_size == 0 and mx_operand.row_is_whole_chunks(K, fia)
              and mx_operand.row_is_whole_chunks(K, fib) and a.numel() > 0 and b.numel() > 0
              and a_scale.shape == a.shape[:-1] + (K // block_size,) and b_scale.shape == b.shape[:-2] + (K // block_size, N))
    if not ok:
        return _fallback(f"matmul operands {fa} x {fb}, shapes {tuple(a.shape)} {tuple(b.shape)}")
    batch = 1
    for d in a.shape[:-2]:
        batch *= d
    if batch > 65535:
        return _fallback("batch > 65535")
    pa = mx_operand.operand(a, mx_operand.ROWS, fia, block_size, batch * M, K)
    if pa is None:
        a3, sa3 = a.contiguous().view(batch, M, K), a_scale.contiguous().view(batch, M, K // block_size)
        pa = _pack(a3, sa3, fia, block_size, batch, M, K, (M * K, K, 1), (sa3.stride(0), sa3.stride(1), 1), check=False)
    pb = mx_operand.operand(b, mx_operand.SECOND, fib, block_size, batch * N, K)      # quantize_mx along axis -2 emitted it
    if pb is None:
        b3, sb3 = b.contiguous().view(batch, K, N), b_scale.contiguous().view(batch, K // block_size, N)
        # second operand: logical rows are b's columns (stride 1), k walks b's rows (stride N)
        pb = _pack(b3, sb3, fib, block_size, batch, N, K, (K * N, 1, N), (sb3.stride(0), 1, sb3.stride(1)), check=False)
    out = torch.empty(a.shape[:-1] + (N,), dtype=a.dtype, device=a.device)
    L = _native.lib()
    _native.check(L.qt_mx_gemm(pa[0].data_ptr(), pa[1].data_ptr(), fia, pb[0].data_ptr(), pb[1].data_ptr(), fib,
                               out.data_ptr(), int(out.dtype == torch.float32), None, batch, M, N, K, M, N,
                               _stream_ptr(a)), "qt_mx_gemm")
    STATS.native += 1
    return out
