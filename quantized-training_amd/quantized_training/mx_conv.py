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
What that route does not take is offered to the integer family next, as linear_mx / matmul_mx do (mx_gemm.py): intN values by their
record or codebook indices with a checked integer codebook, block scales of any value over blocks of 32, 64 or 128 channels.  Both
operands go through qt_mxi_pack -- the weight once as [Cout][kh kw Cin], check on, cached in its own slot; the activation per call
through its strides, check off -- and qt_conv2d_mxi (csrc/qt_mxi_conv.hip) sums every block exactly on the integer matrix cores.
`_int_conv_route_takes` lists the shape classes on which that beat the composite (profiles/conv2d_mxi.txt).

Governed by QT_MX_GEMM like linear_mx / matmul_mx and counted in the same STATS; anything the kernels do not take returns None and
the caller runs the reference formulation."""
import torch

from . import _native, mx_operand
from .fake_quantize import _stream_ptr
from .mx_gemm import (_PAIRS, FMT_ID, STATS, _common_ok, _enabled, _fallback, _int_common_ok, _int_operand_ok, _int_pack, _pack,
                      _pack_rows)

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


def _geometry(input, weight, stride, padding, dilation):
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    h, w = input.shape[2:]
    kh, kw = weight.shape[2:]
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1 if sh > 0 else 0
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1 if sw > 0 else 0
    return sh, sw, ph, pw, dh, dw, ho, wo


def _bias_operand(bias, dtype):
    if bias is None:
        return None
    b = bias.to(dtype).contiguous()
    return b.clone() if b.data_ptr() % 16 else b


def _float_conv2d(input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code, weight_code):
    """The scaled float instruction's route (qt_conv2d_mx): the result, or why not (a string: the counted fallback), or None (never a
    candidate)."""
    if not _common_ok(input, input_scale, input_code, block_size) \
            or not _common_ok(weight, weight_scale, weight_code, block_size) or weight.dtype != input.dtype:
        return None
    if groups != 1 or input.dim() != 4 or weight.dim() != 4 or isinstance(padding, str):
        return f"groups {groups}, input {tuple(input.shape)}, weight {tuple(weight.shape)}, padding {padding}"
    fa, pow2 = mx_operand.format_of(input), (mx_operand.is_pow2(input_scale), mx_operand.is_pow2(weight_scale))
    if fa not in FMT_ID or not all(pow2):
        return f"input format {fa}, power-of-two scales {pow2[0]} {pow2[1]}"
    n, cin, h, w = input.shape
    cout, wcin, kh, kw = weight.shape
    if wcin != cin or cin % 32 or cin % block_size or input.numel() == 0 or weight.numel() == 0:
        return f"Cin = {cin} / {wcin}, block {block_size}"
    nb = cin // block_size
    if tuple(input_scale.shape) != (n, nb, h, w) or tuple(weight_scale.shape) != (cout, nb, kh, kw):
        return f"scale shapes {tuple(input_scale.shape)} {tuple(weight_scale.shape)}"
    sh, sw, ph, pw, dh, dw, ho, wo = _geometry(input, weight, stride, padding, dilation)
    if ho < 1 or wo < 1:
        return f"empty output {ho} x {wo}"
    fid = FMT_ID[fa]
    wop = _conv_weight_operand(weight, weight_scale, block_size)
    if wop is None or (fid, wop[0]) not in _PAIRS or not mx_operand.row_is_whole_chunks(cin, fid):
        return f"weight operand {None if wop is None else wop[0]} with input format {fid}, Cin = {cin}"
    if _APPLY_PACK_RULE and _left_operand(input, fid, block_size) is None and not _pack_route_takes(kh * kw * cin):
        return f"no packed operand on the input and kh kw Cin = {kh * kw * cin} < 128: profiles/conv2d_mx.txt"
    x_codes, x_e8 = _activation_operand(input, input_scale, fid, block_size)
    out = torch.empty((n, cout, ho, wo), dtype=input.dtype, device=input.device, memory_format=torch.channels_last)
    b = _bias_operand(bias, input.dtype)
    rc = _native.lib().qt_conv2d_mx(x_codes.data_ptr(), x_e8.data_ptr(), fid, wop[1].data_ptr(), wop[2].data_ptr(), wop[0],
                                    out.data_ptr(), int(out.dtype == torch.float32), b.data_ptr() if b is not None else None,
                                    n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _stream_ptr(input))
    if _native.declined(rc, dtype=True):
        return f"qt_conv2d_mx declined the shape (code {rc})"
    _native.check(rc, "qt_conv2d_mx")
    STATS.native += 1
    return out


# ---- the integer family: int8 NHWC codes x fp32 block scales (qt_mxi_pack + qt_conv2d_mxi, csrc/qt_mxi_conv.hip) -------------------------
_APPLY_INT_CONV_RULE = True   # tools/exp_conv2d_mxi.py clears it to time the route on the shapes the rule below declines


def _int_conv_route_takes(m, cout, k, taps, dtype):
    """The committed rule, a fixed function of the problem (never a timing): m = N Ho Wo output pixels, k = kh kw Cin the contraction,
    taps = kh kw.  From profiles/conv2d_mxi.txt (ResNet-50 body layers at batch 32, int6 activations under fp8_e5m3 scales over 64
    channels x nf4_6 / int6 weights; the activation pack inside the timed call, the weight operand cached), a class is listed where
    the native median beat the composite's by more than the composite's spread for both weight formats:
      * fp32: every layer whose contraction fills a 128-deep k tile, 1.15-3.45 x the composite's speed; the two 1 x 1 layers over 64
        channels (half a k tile, a pass bound by the bytes it moves, to which the pack adds the input once more) are 0.86-0.97 x;
      * bf16: the 1 x 1 layers with k >= 256 (1.28-2.98 x) and the 3 x 3 layers at 28 x 28 and 14 x 14 (1.51-2.37 x).  The library's
        bf16 convolution keeps k < 256 (0.54-0.98 x) and the 3 x 3 layer at 56 x 56 (0.67-0.72 x); the 3 x 3 layer at 7 x 7 cleared
        the bar by 1.03 x with int6 weights (1.21 x with nf4_6), inside the native route's own spread of 6.5 %, and is not listed.
    Everything else -- other filters above m = 25088 or below 6272 in bf16 among it -- is unmeasured and stays with the composite."""
    if dtype == torch.float32:
        return k >= 128
    return k >= 256 and (taps == 1 or 6272 <= m <= 25088)


def _int_conv_weight_operand(weight, scale, code, block_size):
    """Constant operand [Cout, Cin, kh, kw] (+ scale [Cout, Cin / bs, kh, kw], + codebook) as [Cout][kh kw Cin] int8 codes and
    [Cout][kh kw Cin / bs] fp32 scales: packed once with the check on, cached on the tensor object in the convolution's slot."""
    def pack():
        cout = weight.shape[0]
        w, s = weight.permute(0, 2, 3, 1).contiguous().view(cout, -1), scale.permute(0, 2, 3, 1).contiguous().view(cout, -1)
        return _int_pack(w, s, code, block_size, 1, cout, w.shape[1], (0, w.shape[1], 1), (0, s.shape[1], 1), check=True)
    return mx_operand.int_weight_operand(weight, scale, code, block_size, pack, mx_operand.INT_CONV_SLOT)


def _int_activation_operand(x, scale, code, block_size):
    """NHWC codes [N, H W, Cin] int8 and scales [N, H W, Cin / bs] fp32: qt_mxi_pack through the strides of an NCHW-contiguous or
    channels_last-dense tensor (a .contiguous() first for anything else), check off -- trusted: the record, the codebook."""
    n, c, h, w = x.shape
    xs, ss = _nhwc_strides(x), _nhwc_strides(scale)
    if xs is None:
        x = x.contiguous()
        xs = _nhwc_strides(x)
    if ss is None:
        scale = scale.contiguous()
        ss = _nhwc_strides(scale)
    return _int_pack(x, scale, code, block_size, n, h * w, c, xs, ss, check=False)


def _int_conv2d(input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code, weight_code):
    """The integer family's route (qt_conv2d_mxi): the result, or why not (a string: a pair of integer operands that stays with the
    composite is a counted fallback), or None for every problem that is not this family's."""
    if not (_int_common_ok(input, input_scale, block_size) and _int_common_ok(weight, weight_scale, block_size)) \
            or weight.dtype != input.dtype or not (_int_operand_ok(input, input_code) and _int_operand_ok(weight, weight_code)):
        return None
    if groups != 1 or input.dim() != 4 or weight.dim() != 4 or isinstance(padding, str) or input.numel() == 0 or weight.numel() == 0:
        return f"groups {groups}, input {tuple(input.shape)}, weight {tuple(weight.shape)}, padding {padding}"
    n, cin, h, w = input.shape
    cout, wcin, kh, kw = weight.shape
    if wcin != cin or cin % block_size:
        return f"Cin = {cin} / {wcin}, block {block_size}"
    nb = cin // block_size
    if tuple(input_scale.shape) != (n, nb, h, w) or tuple(weight_scale.shape) != (cout, nb, kh, kw):
        return f"scale shapes {tuple(input_scale.shape)} {tuple(weight_scale.shape)}"
    sh, sw, ph, pw, dh, dw, ho, wo = _geometry(input, weight, stride, padding, dilation)
    if ho < 1 or wo < 1:
        return f"empty output {ho} x {wo}"
    if _APPLY_INT_CONV_RULE and not _int_conv_route_takes(n * ho * wo, cout, kh * kw * cin, kh * kw, input.dtype):
        return f"{n * ho * wo} x {cout} x {kh * kw * cin} in {input.dtype}: not a class of profiles/conv2d_mxi.txt"
    wop = _int_conv_weight_operand(weight, weight_scale, weight_code, block_size)
    if wop is None:
        return "the packer's check refused the weight"
    x_codes, x_scales = _int_activation_operand(input, input_scale, input_code, block_size)
    out = torch.empty((n, cout, ho, wo), dtype=input.dtype, device=input.device, memory_format=torch.channels_last)
    b = _bias_operand(bias, input.dtype)
    rc = _native.lib().qt_conv2d_mxi(x_codes.data_ptr(), x_scales.data_ptr(), wop[0].data_ptr(), wop[1].data_ptr(), block_size,
                                     out.data_ptr(), int(out.dtype == torch.float32), b.data_ptr() if b is not None else None,
                                     n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, _stream_ptr(input))
    if _native.declined(rc):
        return f"qt_conv2d_mxi declined the shape (code {rc})"
    _native.check(rc, "qt_conv2d_mxi")
    STATS.native += 1
    return out


def mx_conv2d_or_none(input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code,
                      weight_code):
    """conv2d_mx through qt_conv2d_mx or qt_conv2d_mxi -- a channels_last tensor of logical shape [N, Cout, Ho, Wo] in the input's
    dtype -- or None.  The float family first, unchanged; the integer family where that one does not take the call; one counted
    fallback for a call that either family looked at as its own and neither took; nothing for a call that is neither's."""
    if not _enabled():
        return None
    args = (input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code, weight_code)
    res = _float_conv2d(*args)
    if isinstance(res, torch.Tensor):
        return res
    out = _int_conv2d(*args)
    if isinstance(out, torch.Tensor):
        return out
    why = out if out is not None else res
    return _fallback(why) if why is not None else None
