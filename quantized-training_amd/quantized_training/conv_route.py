"""Route of a QAT Conv2d's convolution on the device: the in-tree implicit-GEMM kernel (csrc/qt_conv.hip, qt_conv2d_bf16) or the
library's convolution (torch -> MIOpen), decided per problem and recorded for fused.routes_report().

    QT_CONV_GEMM=auto   by the committed rule (_auto_takes: the shape classes on which the kernel measured at least as fast as the
                        library, profiles/conv2d_routes.txt) -- the default
    QT_CONV_GEMM=0      never
    QT_CONV_GEMM=1      wherever the kernel takes the shape

The weight handed in is what the twin's weight fake-quantizer returned; nothing here quantizes.  A forward through the kernel costs: one
copy of the input to channels_last when it does not arrive so (the result IS channels_last, so BN / ReLU / pooling keep the format and
only the first routed layer of a model pays it), one copy of the small quantized weight to [Cout][kh][kw][Cin], one kernel launch."""
import ctypes

import torch

from . import switches

__all__ = ["conv2d_or_none", "conv_gemm_mode", "CONV_ROUTES"]

CONV_ROUTES = {}          # "conv2d N×Cin×H×W → Cout k s p d" -> "in_tree_bf16_conv" | "library_conv" (fused.routes_report)


def conv_gemm_mode():
    return switches.mode("QT_CONV_GEMM")


def _pair_str(v):
    return v if isinstance(v, str) else f"{v[0]}x{v[1]}"


def _route_key(x, wq, stride, padding, dilation, groups):
    n, cin, h, w = x.shape
    key = f"conv2d {n}×{cin}×{h}×{w} → {wq.shape[0]} k{wq.shape[2]}x{wq.shape[3]} s{_pair_str(stride)} p{_pair_str(padding)} d{_pair_str(dilation)}"
    return key if groups == 1 else key + f" g{groups}"


def _resolve_padding(padding, kernel, stride, dilation):
    """Integer padding of a string padding, or None where it has none ('same' with an odd total: torch pads one side more)."""
    if not isinstance(padding, str):
        return tuple(int(p) for p in padding)
    if padding == "valid":
        return (0, 0)
    if padding == "same" and all(s == 1 for s in stride):
        total = [d * (k - 1) for d, k in zip(dilation, kernel)]
        if all(t % 2 == 0 for t in total):
            return tuple(t // 2 for t in total)
    return None


def _auto_takes(m, k_tiles):
    """The committed rule of QT_CONV_GEMM=auto, a fixed function of the shape (never a timing: every process and rank routes a shape the
    same way): m = N Ho Wo output pixels, k_tiles = kh kw Cin / 64.  From profiles/conv2d_routes.txt (ResNet-50 body layers, batch 32;
    DESIGN 4.3e): with the weight copy of the route counted, the kernel is 1.3-4.4 x the library's speed on every 3 x 3 layer and every
    1 x 1 layer with Cin >= 512 (eight k tiles or more), and on the 1 x 1 layers with Cin = 256 over small planes; over 56 x 56 and
    28 x 28 planes the 1 x 1 layers with Cin <= 256 are a store-bound pass that the library runs as fast or faster (0.75-1.2 x): those stay
    with the library."""
    return k_tiles >= 8 or (k_tiles >= 4 and m <= 8192)


def _plan(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw):
    """(output pixels, k tiles) when qt_conv2d_bf16 takes the shape, else None."""
    from . import _native
    tiles_m, tile_m, k_tiles = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if _native.lib().qt_conv2d_plan(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, ctypes.byref(tile_m), None, ctypes.byref(tiles_m), None,
                                    ctypes.byref(k_tiles)) != 0:
        return None
    ho = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (w + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    return n * ho * wo, k_tiles.value


def _launch(xc, wk, bias, stride, padding, dilation):
    """qt_conv2d_bf16 on a channels_last input and a [Cout][kh][kw][Cin] weight; the channels_last result, or None when declined."""
    from . import _native
    n, cin, h, w = xc.shape
    cout, _, kh, kw = wk.shape
    ho = (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    wo = (w + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    if ho < 1 or wo < 1:
        return None
    y = torch.empty((n, cout, ho, wo), dtype=torch.bfloat16, device=xc.device, memory_format=torch.channels_last)
    _native.note_device(xc.device.index)
    rc = _native.lib().qt_conv2d_bf16(xc.data_ptr(), wk.data_ptr(), bias.data_ptr() if bias is not None else None, y.data_ptr(),
                                      n, h, w, cin, cout, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1],
                                      ctypes.c_void_p(torch.cuda.current_stream(xc.device).cuda_stream))
    if _native.declined(rc):
        return None
    _native.check(rc, "qt_conv2d_bf16")
    return y


def _is_nhwc_dense(t):
    return t.permute(0, 2, 3, 1).is_contiguous()


def _nhwc_dense(t):
    """`t` [N, C, H, W] as dense NHWC memory (a copy only when it is not already)."""
    return t if _is_nhwc_dense(t) else t.contiguous(memory_format=torch.channels_last)


class _Conv2dInTree(torch.autograd.Function):
    """Forward on the in-tree kernel; backward is the library's (aten.convolution_backward on the saved input and quantized weight)."""

    @staticmethod
    def forward(ctx, x, wq, bias, stride, padding, dilation):
        xc = _nhwc_dense(x)
        y = _launch(xc, _nhwc_dense(wq), bias, stride, padding, dilation)
        if y is None:
            raise RuntimeError("qt_conv2d_bf16 declined a problem its plan took")
        ctx.save_for_backward(xc, wq)
        ctx.conv = (stride, padding, dilation, None if bias is None else tuple(bias.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, wq = ctx.saved_tensors
        stride, padding, dilation, bias_shape = ctx.conv
        mask = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias_shape is not None and ctx.needs_input_grad[2]]
        gx, gw, gb = torch.ops.aten.convolution_backward(gy, xc, wq, bias_shape, list(stride), list(padding), list(dilation), False, [0, 0], 1, mask)
        return (gx if mask[0] else None, gw if mask[1] else None, gb if mask[2] else None, None, None, None)


def conv2d_or_none(x, wq, bias, stride, padding, dilation, groups):
    """F.conv2d(x, wq, bias, ...) through the in-tree kernel -- a channels_last tensor of the usual logical shape -- or None where the
    library keeps the problem (the caller then runs torch's convolution).  Every decision is recorded in CONV_ROUTES."""
    if not x.is_cuda or x.dim() != 4 or wq.dim() != 4:
        return None
    stride, dilation = tuple(stride), tuple(dilation)
    pad = _resolve_padding(padding, wq.shape[2:], stride, dilation)
    key = _route_key(x, wq, stride, pad if pad is not None else padding, dilation, groups)
    n, cin, h, w = x.shape
    cout, _, kh, kw = wq.shape
    mode = conv_gemm_mode()
    ok = (mode != "0" and pad is not None and groups == 1 and wq.shape[1] == cin
          and x.dtype == torch.bfloat16 and wq.dtype == torch.bfloat16 and wq.device == x.device
          and (bias is None or (bias.dtype == torch.bfloat16 and bias.is_contiguous() and bias.numel() == cout and bias.data_ptr() % 8 == 0
                                and bias.device == x.device)))
    if ok:
        plan = _plan(n, h, w, cin, cout, kh, kw, stride[0], stride[1], pad[0], pad[1], dilation[0], dilation[1])
        ok = plan is not None and (mode == "1" or _auto_takes(*plan))
    if ok and _is_nhwc_dense(x) and x.data_ptr() % 16 != 0:
        ok = False                                        # a view at an odd offset that would be read as it stands
    if not ok:
        CONV_ROUTES.setdefault(key, "library_conv")
        return None
    CONV_ROUTES.setdefault(key, "in_tree_bf16_conv")
    if torch.is_grad_enabled() and (x.requires_grad or wq.requires_grad or (bias is not None and bias.requires_grad)):
        return _Conv2dInTree.apply(x, wq, bias, stride, pad, dilation)
    y = _launch(_nhwc_dense(x), _nhwc_dense(wq), bias, stride, pad, dilation)
    if y is None:
        raise RuntimeError("qt_conv2d_bf16 declined a problem its plan took")
    return y
