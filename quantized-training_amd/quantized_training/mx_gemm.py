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

What that route does not take is offered to the integer family next (qt_mxi_pack + qt_mxi_gemm): operands whose
values are integers -- by the record an `intN` map (N <= 8) left on them, or as indices that come with a codebook
of at most 256 integer levels in [-128, 127] (checked once per codebook on the host, cached on the tensor by
version) -- under block scales of ANY finite positive value (fp8_e5m3, amax / qmax, powers of two) over blocks of
32, 64 or 128 elements, bf16 or fp32.  Each block is summed exactly in int32 on the integer matrix cores and
multiplied by the fp32 product of its two scales; one rounding at the end.  A weight is packed once with the
packer's check on and cached in its own slot (mx_operand.int_weight_operand); activations are packed per call
with the check off, trusting record and codebook.  _int_route_takes keeps the shape classes with the composite
on which the kernel did not beat it (profiles/mx_int_gemm.txt).

Anything else -- mixed float x integer pairs, nf4's fractional levels, block size 16 or above 128, tuple block
sizes, fp16, codebooks above 256 entries, an integer activation without record or codebook -- returns None, is
counted as a fallback, and the caller runs the reference formulation; so do CPU tensors, which never get here.
QT_MX_GEMM=0 disables both native families.
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


def _float_linear(input, weight, bias, input_scale, weight_scale, block_size, input_code, weight_code):
    """The scaled float instruction's route: the result, or why not (a string: today's counted fallback), or None (never a candidate)."""
    if not _common_ok(input, input_scale, input_code, block_size) \
            or not _common_ok(weight, weight_scale, weight_code, block_size) or weight.dtype != input.dtype:
        return None
    fa, pow2 = mx_operand.format_of(input), mx_operand.is_pow2(input_scale)
    if fa not in FMT_ID or not pow2 or weight.dim() != 2 or input.dim() < 2:
        return f"input format {fa}, power-of-two scale {pow2}"
    K = input.shape[-1]
    N = weight.shape[0]
    if weight.shape[1] != K or K % 32 or K % block_size or input.numel() == 0:
        return f"K = {K}, block {block_size}"
    wop = _weight_operand(weight, weight_scale, block_size)
    fid = FMT_ID[fa]
    if wop is None or (fid, wop[0]) not in _PAIRS or not mx_operand.row_is_whole_chunks(K, fid):
        return f"weight operand {None if wop is None else wop[0]} with input format {fid}, K = {K}"
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


def _float_matmul(a, b, a_scale, b_scale, block_size, a_code, b_code):
    """a [..., M, K] with blocks along K (last axis); b [..., K, N] with blocks along K (axis -2).  Returns as _float_linear."""
    if not _common_ok(a, a_scale, a_code, block_size) or not _common_ok(b, b_scale, b_code, block_size) \
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
        return f"matmul operands {fa} x {fb}, shapes {tuple(a.shape)} {tuple(b.shape)}"
    batch = 1
    for d in a.shape[:-2]:
        batch *= d
    if batch > 65535:
        return "batch > 65535"
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


# ---- the integer family: int8 codes x fp32 block scales (qt_mxi_pack + qt_mxi_gemm) ------------------------------------------------
def _on_device(t):
    return t.device.type == "cuda"


def _int_common_ok(x, scale, block_size):
    return (scale is not None and isinstance(block_size, int) and not isinstance(block_size, bool) and block_size in mx_operand.INT_BLOCKS
            and x.dtype in (torch.bfloat16, torch.float32) and scale.dtype == x.dtype and _on_device(x) and scale.device == x.device)


def _int_operand_ok(x, code):
    """Integer-valued by the record its producer left, or indices that come with an integer codebook (checked once per codebook)."""
    if code is None:
        return mx_operand.int_format_of(x) is not None
    return code.dtype == x.dtype and code.device == x.device and mx_operand.int_codebook_ok(code)


_APPLY_INT_RULE = True        # tools/exp_mx_int_gemm.py clears it to time the route on the shapes the rule below declines


def _int_route_takes(m, n, k, batch, block_size, dtype):
    """The committed rule, a fixed function of the problem (never a timing).  From profiles/mx_int_gemm.txt (activation pack inside the
    timed call, weight operand cached): in fp32 the integer GEMM is 2.5-4.1 x the composite's speed on LLaMA-2-7B's projections,
    1.1-1.4 x on the attention matmuls and 1.3-2.5 x on smaller Linears -- every measured row, so fp32 always goes native.  In bf16 it
    wins every row up to 512 x 1024 x 1024 = 2^29 multiply-adds (1.7 x while the call is bound by its launches, the composite's
    five against two; 1.2 x at 2^29) and loses the projections (0.52-1.04 x) and the attention matmuls (0.55-0.72 x), 2^32 and
    more, to the library's bf16 GEMM, the register-staged kernel being paced by the latency of its k steps there: bf16 problems
    above 2^29 multiply-adds stay with the composite."""
    return dtype == torch.float32 or batch * m * n * k <= (1 << 29)


def _int_pack(values, scale, code, block_size, batch, rows, K, x_strides, s_strides, check):
    """-> (codes [batch, rows, K] int8, scales [batch, rows, K / bs] fp32) or None when the packer's check refuses."""
    L = _native.lib()
    dev = values.device
    codes = torch.empty((batch, rows, K), dtype=torch.int8, device=dev)
    scales = torch.empty((batch, rows, K // block_size), dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev) if check else None
    c = code.contiguous() if code is not None else None
    _native.check(L.qt_mxi_pack(values.data_ptr(), scale.data_ptr(), int(values.dtype == torch.float32),
                                c.data_ptr() if c is not None else None, c.numel() if c is not None else 0, codes.data_ptr(),
                                scales.data_ptr(), batch, rows, K, *x_strides, *s_strides, block_size,
                                bad.data_ptr() if check else None, _stream_ptr(values)), "qt_mxi_pack")
    if check and int(bad.item()) != 0:
        return None
    return codes, scales


def _int_weight_operand(weight, scale, code, block_size):
    """Constant operand [N, K] (+ scale [N, K / bs], + codebook): packed once with the check on, cached on the tensor object."""
    def pack():
        w, s = weight.contiguous(), scale.contiguous()
        rows, K = w.shape
        return _int_pack(w, s, code, block_size, 1, rows, K, (0, K, 1), (0, s.shape[-1], 1), check=True)
    return mx_operand.int_weight_operand(weight, scale, code, block_size, pack)


def _int_gemm(pa, pb, block_size, out, bias, batch, M, N, K, a_rows, b_rows, ref):
    L = _native.lib()
    _native.check(L.qt_mxi_gemm(pa[0].data_ptr(), pa[1].data_ptr(), pb[0].data_ptr(), pb[1].data_ptr(), block_size, out.data_ptr(),
                                int(out.dtype == torch.float32), bias.data_ptr() if bias is not None else None, batch, M, N, K,
                                a_rows, b_rows, _stream_ptr(ref)), "qt_mxi_gemm")
    STATS.native += 1
    return out


def _int_linear(input, weight, bias, input_scale, weight_scale, block_size, input_code, weight_code):
    """The result, or None for every problem that is not the integer family's."""
    if not (_int_common_ok(input, input_scale, block_size) and _int_common_ok(weight, weight_scale, block_size)) \
            or weight.dtype != input.dtype or weight.dim() != 2 or input.dim() < 2 or input.numel() == 0 or weight.numel() == 0:
        return None
    K, N = input.shape[-1], weight.shape[0]
    if weight.shape[1] != K or K % block_size or K % 16:
        return None
    nb = K // block_size
    if tuple(input_scale.shape) != tuple(input.shape[:-1]) + (nb,) or tuple(weight_scale.shape) != (N, nb):
        return None
    if not (_int_operand_ok(input, input_code) and _int_operand_ok(weight, weight_code)):
        return None
    M = input.numel() // K
    if _APPLY_INT_RULE and not _int_route_takes(M, N, K, 1, block_size, input.dtype):
        return None
    wop = _int_weight_operand(weight, weight_scale, weight_code, block_size)
    if wop is None:
        return None
    x, s = input.contiguous(), input_scale.contiguous()
    pa = _int_pack(x, s, input_code, block_size, 1, M, K, (0, K, 1), (0, nb, 1), check=False)     # trusted: the record, the codebook
    out = torch.empty(input.shape[:-1] + (N,), dtype=input.dtype, device=input.device)
    b = bias.to(input.dtype).contiguous() if bias is not None else None
    return _int_gemm(pa, wop, block_size, out, b, 1, M, N, K, 0, 0, x)


def _rows_view(t, batch, rows, cols):
    """[..., cols, rows] seen as `rows` logical rows of `cols`: (tensor, (batch, row, k) element strides) without a copy where the
    tensor is a transposed view of contiguous storage (the Q . K^T case), else over a contiguous copy."""
    tt = t.transpose(-1, -2)
    if tt.is_contiguous():
        return tt, (rows * cols, cols, 1)
    return t.contiguous(), (cols * rows, 1, rows)


def _int_matmul(a, b, a_scale, b_scale, block_size, a_code, b_code):
    if not (_int_common_ok(a, a_scale, block_size) and _int_common_ok(b, b_scale, block_size)) or a.dtype != b.dtype \
            or a.dim() < 2 or b.dim() < 2 or a.shape[:-2] != b.shape[:-2] or a.shape[-1] != b.shape[-2] or a.numel() == 0 or b.numel() == 0:
        return None
    M, K = a.shape[-2:]
    N = b.shape[-1]
    if K % block_size or K % 16:
        return None
    nb = K // block_size
    if tuple(a_scale.shape) != tuple(a.shape[:-1]) + (nb,) or tuple(b_scale.shape) != tuple(b.shape[:-2]) + (nb, N):
        return None
    batch = 1
    for d in a.shape[:-2]:
        batch *= d
    if batch > 65535 or not (_int_operand_ok(a, a_code) and _int_operand_ok(b, b_code)):
        return None
    if _APPLY_INT_RULE and not _int_route_takes(M, N, K, batch, block_size, a.dtype):
        return None
    a3, sa3 = a.contiguous(), a_scale.contiguous()
    pa = _int_pack(a3, sa3, a_code, block_size, batch, M, K, (M * K, K, 1), (M * nb, nb, 1), check=False)
    b3, xb = _rows_view(b, batch, N, K)               # second operand: logical rows are b's columns, k walks b's rows
    sb3, xs = _rows_view(b_scale, batch, N, nb)
    pb = _int_pack(b3, sb3, b_code, block_size, batch, N, K, xb, xs, check=False)
    out = torch.empty(a.shape[:-1] + (N,), dtype=a.dtype, device=a.device)
    return _int_gemm(pa, pb, block_size, out, None, batch, M, N, K, M, N, a3)


# ---- the operators' entry points ---------------------------------------------------------------------------------------------------
def _route(float_route, int_route, args):
    """The float family first, unchanged; the integer family where that one does not take the call; else one counted fallback."""
    if not _enabled():
        return None
    res = float_route(*args)
    if isinstance(res, torch.Tensor):
        return res
    out = int_route(*args)
    if out is not None:
        return out
    return _fallback(res if res is not None else "not an operand pair of either native family")


def mx_linear_or_none(input, weight, bias, input_scale, weight_scale, block_size, input_code, weight_code):
    return _route(_float_linear, _int_linear, (input, weight, bias, input_scale, weight_scale, block_size, input_code, weight_code))


def mx_matmul_or_none(a, b, a_scale, b_scale, block_size, a_code, b_code):
    return _route(_float_matmul, _int_matmul, (a, b, a_scale, b_scale, block_size, a_code, b_code))
