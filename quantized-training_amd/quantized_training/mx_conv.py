"""conv2d_mx on gfx950's block-scaled matrix instruction (upstream decomposed.py:265-301).

The reference states the op as "multiply each operand by its block scales expanded along the channel axis, then F.conv2d".  For the
operands mx_gemm takes (element values in one of the five formats of v_mfma_scale_f32_16x16x128_f8f6f4, power-of-two scales over
blocks of a multiple of 32 channels) the same sum is computed by qt_conv2d_mx (csrc/qt_mx_conv.hip), an implicit GEMM that gathers
the element codes and E8M0 bytes of each filter tap from NHWC operands: no dequantized copy of either operand is ever written.

Weight [Cout, Cin, kh, kw]: packed once as [Cout][kh kw Cin] with the packer's check on, cached on the tensor object.
Activation, in this order:
  1. the NHWC operand quantize_mx left on its result (mx_operand.NHWC: the strided pass over a contiguous NCHW tensor, or the
     last-axis pass over the stored tensor of a channels_last one);
  2. qt_mx_pack addressed through strides (batch N, rows H W, k = C) for NCHW-contiguous or channels_last-dense values and scales,
     after a .contiguous() for any other layout.  One measured shape class does not pay for that pack and stays with the composite
     when no operand was left (`_pack_route_takes`, profiles/conv2d_mx.txt).
Governed by QT_MX_GEMM like linear_mx / matmul_mx and counted in the same STATS; anything the kernel does not take returns None and
the caller runs the reference formulation."""
import torch

from . import _native, mx_operand
from .fake_quantize import _stream_ptr
from .mx_gemm import _PAIRS, FMT_ID, STATS, _common_ok, _enabled, _fallback, _pack, _pack_rows

__all__ = ["mx_conv2d_or_none", "STATS"]


def _pair(v):
    if isinstance(v, int):
        return (v, v)
    v = tuple(int(e) for e in v)
    return v * 2 if len(v) == 1 else v


def _conv_weight_operand(weight, scale, block_size):
    """Constant operand [Cout, Cin, kh, kw] (+ scale [Cout, Cin / bs, kh, kw]) as [Cout][kh kw Cin]: packed once, cached on the tensor
    object -> (format id, codes, e8m0) or None when the packer refuses it in every format."""
    cout, cin = weight.shape[:2]
    return mx_operand.weight_operand(weight, scale, block_size, mx_operand.CONV_SLOT,
                                     lambda: (weight.permute(0, 2, 3, 1).contiguous().view(cout, -1),
                                              scale.permute(0, 2, 3, 1).contiguous().view(cout, -1)), cin, _pack_rows)


def _nhwc_strides(t):
    """(batch, row, k) element strides of the [N, H W, C] view of a 4-D tensor that is NCHW-contiguous or channels_last-dense, else None."""
    n, c, h, w = t.shape
    if t.is_contiguous():
        return (c * h * w, 1, h * w)
    if t.permute(0, 2, 3, 1).is_contiguous():
        return (h * w * c, c, 1)
    return None


def _left_operand(x, fid, block_size):
    """The NHWC operand quantize_mx left on `x`, (codes, e8m0), when format, block size and shape match; else None."""
    n, c, h, w = x.shape
    return mx_operand.operand(x, mx_operand.NHWC, fid, block_size, n * h * w, c)


_APPLY_PACK_RULE = True       # tools/exp_conv2d_mx.py clears it to time the route the rule below declines


def _pack_route_takes(k):
    """The committed rule for an activation that arrives WITHOUT a packed operand, so that qt_mx_pack has to run in front of the kernel; a
    fixed function of the shape (never a timing): k = kh kw Cin, the contraction.  From profiles/conv2d_mx.txt (ResNet-50 body layers,
    batch 32, fp8 and fp4): with the operand quantize_mx leaves, the kernel is 1.12-9.2 x the composite's speed on all
    thirteen layers and never declines.  With the pack inside the call it is 1.02-3.1 x on every layer whose contraction fills at
    least one 128-deep k tile (128 -> 512 1 x 1 in fp8: 0.99 x, inside the composite's 5 % spread), but on the two 1 x 1 layers over
    64 channels -- half a k tile: a pass bound by the bytes it moves, to which the pack adds the input once more -- it is 0.76 x
    (fp8) / 0.79 x (fp4) into 256 channels and 0.88 x / 0.92 x into 64, outside the composite's spread.  Contractions under one k
    tile therefore stay with the composite when no operand was left."""
    return k >= 128


def _activation_operand(x, scale, fid, block_size):
    """NHWC codes [N H W, Cin bits / 8] and E8M0 bytes [N H W, Cin / 32] of a quantize_mx result."""
    n, c, h, w = x.shape
    pre = _left_operand(x, fid, block_size)
    if pre is not None:
        return pre
    xs, ss = _nhwc_strides(x), _nhwc_strides(scale)
    if xs is None:
        x, xs = x.contiguous(), (c * h * w, 1, h * w)
    if ss is None:
        scale = scale.contiguous()
        ss = _nhwc_strides(scale)
    codes, e8 = _pack(x, scale, fid, block_size, n, h * w, c, xs, ss, check=False)
    return codes.view(n * h * w, -1), e8.view(n * h * w, -1)


def mx_conv2d_or_none(input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code,
                      weight_code):
    """conv2d_mx through qt_conv2d_mx -- a channels_last tensor of logical shape [N, Cout, Ho, Wo] in the input's dtype -- or None."""
    if not _enabled() or not _common_ok(input, input_scale, input_code, block_size) \
            or not _common_ok(weight, weight_scale, weight_code, block_size) or weight.dtype != input.dtype:
        return None
    if groups != 1 or input.dim() != 4 or weight.dim() != 4 or isinstance(padding, str):
        return _fallback(f"groups {groups}, input {tuple(input.shape)}, weight {tuple(weight.shape)}, padding {padding}")
    fa, pow2 = mx_operand.format_of(input), (mx_operand.is_pow2(input_scale), mx_operand.is_pow2(weight_scale))
    if fa not in FMT_ID or not all(pow2):
        return _fallback(f"input format {fa}, power-of-two scales {pow2[0]} {pow2[1]}")
    n, cin, h, w = input.shape
    cout, wcin, kh, kw = weight.shape
    if wcin != cin or cin % 32 or cin % block_size or input.numel() == 0 or weight.numel() == 0:
        return _fallback(f"Cin = {cin} / {wcin}, block {block_size}")
    nb = cin // block_size
    if tuple(input_scale.shape) != (n, nb, h, w) or tuple(weight_scale.shape) != (cout, nb, kh, kw):
        return _fallback(f"scale shapes {tuple(input_scale.shape)} {tuple(weight_scale.shape)}")
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1 if sh > 0 else 0
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1 if sw > 0 else 0
    if ho < 1 or wo < 1:
        return _fallback(f"empty output {ho} x {wo}")
    fid = FMT_ID[fa]
    wop = _conv_weight_operand(weight, weight_scale, block_size)
    if wop is None or (fid, wop[0]) not in _PAIRS or not mx_operand.row_is_whole_chunks(cin, fid):
        return _fallback(f"weight operand {None if wop is None else wop[0]} with input format {fid}, Cin = {cin}")
    if _APPLY_PACK_RULE and _left_operand(input, fid, block_size) is None and not _pack_route_takes(kh * kw * cin):
        return _fallback(f"no packed operand on the input and kh kw Cin = {kh * kw * cin} < 128: profiles/conv2d_mx.txt")
    x_codes, x_e8 = _activation_operand(input, input_scale, fid, block_size)
    out = torch.empty((n, cout, ho, wo), dtype=input.dtype, device=input.device, memory_format=torch.channels_last)
    b = None
    if bias is not None:
        b = bias.to(input.dtype).contiguous()
        if b.data_ptr() % 16:
            b = b.clone()
    rc = _native.lib().qt_conv2d_mx(x_codes.data_ptr(), x_e8.data_ptr(), fid, wop[1].data_ptr(), wop[2].data_ptr(), wop[0],
                                    out.data_ptr(), int(out.dtype == torch.float32), b.data_ptr() if b is not None else None,
                                    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _stream_ptr(input))
    if _native.declined(rc, dtype=True):
        return _fallback(f"qt_conv2d_mx declined the shape (code {rc})")
    _native.check(rc, "qt_conv2d_mx")
    STATS.native += 1
    return out
