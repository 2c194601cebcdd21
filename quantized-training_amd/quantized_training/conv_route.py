"""Route of a QAT Conv2d's convolution on the device: the in-tree implicit-GEMM kernels (csrc/qt_conv.hip, qt_conv2d_bf16, and for the
backward csrc/qt_conv_backward.hip, qt_conv2d_dgrad_bf16 / qt_conv2d_wgrad_bf16) or the library's convolution (torch -> MIOpen), decided
per problem and per product and recorded for fused.routes_report().

    QT_CONV_GEMM=auto   by the committed rules, fixed functions of the shape: the forward by _auto_takes (the shape classes on which the
                        kernel measured at least as fast as the library, profiles/conv2d_routes.txt); the input gradient and the weight
                        gradient of a problem whose forward went in-tree each by a rule of their own (_auto_takes_dgrad,
                        _auto_takes_wgrad: in-tree only where a committed table of tools/exp_conv2d_backward.py backs it) -- the default
    QT_CONV_GEMM=0      never: the library for everything
    QT_CONV_GEMM=1      wherever a kernel takes the shape, forward and backward

The backward is only considered for problems whose forward went in-tree (that is where the autograd Function below exists).  Whatever
product stays with the library is computed by ONE aten.convolution_backward with the matching output mask; when all the requested
products go in-tree the library is not called.  The bias gradient needs no kernel of its own: it is qt_colsum_bf16 on the
[N Ho Wo][Cout] view of the gradient (torch's sum where that kernel's contract does not fit), unless every other requested product is
the library's -- its call then returns the bias gradient as well, as it always did.

The weight handed in is what the twin's weight fake-quantizer returned; nothing here quantizes.  A forward through the kernel costs: one
copy of the input to channels_last when it does not arrive so (the result IS channels_last, so BN / ReLU / pooling keep the format and
only the first routed layer of a model pays it), one copy of the small quantized weight to [Cout][kh][kw][Cin], one kernel launch."""
import ctypes

import torch

from . import switches

__all__ = ["conv2d_or_none", "conv_gemm_mode", "CONV_ROUTES"]

# "conv2d N×Cin×H×W → Cout k s p d" -> "in_tree_bf16_conv" | "library_conv" (fused.routes_report); the backward products of a problem
# are recorded under the same description behind "conv2d_dgrad" / "conv2d_wgrad" when a backward first computes them
CONV_ROUTES = {}


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


def _auto_takes_dgrad(m_in, cin, k_tiles):
    """The committed rule of QT_CONV_GEMM=auto for the input gradient, a fixed function of the shape: m_in = N H W input pixels (the rows
    of the product), cin its columns, k_tiles = kh kw Cout / 64.  A class goes in-tree only where the committed table of
    tools/exp_conv2d_backward.py (profiles/conv2d_bwd_routes.txt) shows the kernel faster than the library's single-product backward by
    more than the library's run-to-run spread.  The table has the kernel at 1.2-2.2 x on eleven of thirteen layers, but its spread is
    104 % (single repeats of the library's 1 x 1 input gradient took twice their median) and no class clears that: every
    class stays with the library."""
    return False


def _auto_takes_wgrad(m, cout, cols, ksplit):
    """The same for the weight gradient: m = N Ho Wo output pixels (the contraction), cout x cols = Cout x kh kw Cin the output, ksplit the
    split factor of qt_conv2d_backward_plan on an MI355X (256 CUs).  The table has the kernel at 2.0-3.7 x on planes up to 28 x 28 and
    0.82-2.0 x over 56 x 56; against the same 104 % spread no class clears the bar as a whole: every class stays with the library."""
    return False


def backward_plan(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw):
    """(dgrad, wgrad) as _native.QtConv2dProductPlan when qt_conv2d_dgrad_bf16 / qt_conv2d_wgrad_bf16 take the shape, else None."""
    from . import _native
    d, g = _native.QtConv2dProductPlan(), _native.QtConv2dProductPlan()
    if _native.lib().qt_conv2d_backward_plan(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, ctypes.byref(d), ctypes.byref(g)) != 0:
        return None
    return d, g


def _backward_routes(mode, n, h, w, cin, cout, kh, kw, stride, padding, dilation):
    """(dgrad in-tree?, wgrad in-tree?) of a problem whose forward went in-tree under `mode` ("1" or "auto")."""
    plan = backward_plan(n, h, w, cin, cout, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1])
    if plan is None:
        return False, False
    d, g = plan
    if mode == "1":
        return bool(d.taken), bool(g.taken)
    ho = (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    wo = (w + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    return (bool(d.taken) and _auto_takes_dgrad(n * h * w, cin, d.k_tiles),
            bool(g.taken) and _auto_takes_wgrad(n * ho * wo, cout, kh * kw * cin, g.ksplit))


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


def _conv_ints(xc, wk, stride, padding, dilation):
    n, cin, h, w = xc.shape
    cout, _, kh, kw = wk.shape
    return (n, h, w, cin, cout, kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1])


def _launch_dgrad(gyc, wk, xc, stride, padding, dilation):
    """qt_conv2d_dgrad_bf16 on an NHWC-dense gradient and a [Cout][kh][kw][Cin] weight: the channels_last input gradient, or None."""
    from . import _native
    gx = torch.empty(xc.shape, dtype=torch.bfloat16, device=gyc.device, memory_format=torch.channels_last)
    _native.note_device(gyc.device.index)
    rc = _native.lib().qt_conv2d_dgrad_bf16(gyc.data_ptr(), wk.data_ptr(), gx.data_ptr(), *_conv_ints(xc, wk, stride, padding, dilation),
                                            ctypes.c_void_p(torch.cuda.current_stream(gyc.device).cuda_stream))
    if _native.declined(rc):
        return None
    _native.check(rc, "qt_conv2d_dgrad_bf16")
    return gx


def _launch_wgrad(gyc, xc, wk, stride, padding, dilation):
    """qt_conv2d_wgrad_bf16: the weight gradient with the weight's logical shape over [Cout][kh][kw][Cin] memory, or None."""
    from . import _native, fused
    ints = _conv_ints(xc, wk, stride, padding, dilation)
    plan = backward_plan(*ints)
    if plan is None or not plan[1].taken:
        return None
    g = plan[1]
    ws = tickets = None
    if g.ksplit > 1:
        ws, tickets = fused.splitk_scratch("conv_wgrad", g.ws_bytes, g.n_tickets, gyc.device)
    cout, cin, kh, kw = wk.shape
    gw = torch.empty((cout, kh, kw, cin), dtype=torch.bfloat16, device=gyc.device)
    _native.note_device(gyc.device.index)
    rc = _native.lib().qt_conv2d_wgrad_bf16(gyc.data_ptr(), xc.data_ptr(), gw.data_ptr(), *ints,
                                            ws.data_ptr() if ws is not None else None, ws.numel() * 4 if ws is not None else 0,
                                            tickets.data_ptr() if tickets is not None else None, tickets.numel() if tickets is not None else 0,
                                            ctypes.c_void_p(torch.cuda.current_stream(gyc.device).cuda_stream))
    if _native.declined(rc):
        return None
    _native.check(rc, "qt_conv2d_wgrad_bf16")
    return gw.permute(0, 3, 1, 2)


def _library_backward(gy, xc, wq, bias_shape, stride, padding, dilation, mask):
    """The products `mask` names from the library (what the reference's autograd runs for all three)."""
    return torch.ops.aten.convolution_backward(gy, xc, wq, bias_shape, list(stride), list(padding), list(dilation), False, [0, 0], 1, mask)


def _bias_grad(gyc):
    """Column sums of the [N Ho Wo][Cout] view of an NHWC-dense gradient: qt_colsum_bf16 (fp32 sums in a fixed order, one rounding) where
    its contract fits, torch's sum otherwise."""
    from . import _native
    n, cout, ho, wo = gyc.shape
    if cout % 8 == 0 and gyc.data_ptr() % 16 == 0 and gyc.numel() > 0:
        gb = torch.empty((cout,), dtype=torch.bfloat16, device=gyc.device)
        _native.note_device(gyc.device.index)
        rc = _native.lib().qt_colsum_bf16(gyc.data_ptr(), gb.data_ptr(), n * ho * wo, cout,
                                          ctypes.c_void_p(torch.cuda.current_stream(gyc.device).cuda_stream))
        if not _native.declined(rc):
            _native.check(rc, "qt_colsum_bf16")
            return gb
    return gyc.sum((0, 2, 3))


class _Conv2dInTree(torch.autograd.Function):
    """Forward on the in-tree kernel; each backward product on its in-tree kernel or the library's (aten.convolution_backward on the
    saved input and quantized weight, with an output mask for what stays there), as decided at forward time by `bwd`."""

    @staticmethod
    def forward(ctx, x, wq, bias, stride, padding, dilation, bwd):
        xc = _nhwc_dense(x)
        wk = _nhwc_dense(wq)
        y = _launch(xc, wk, bias, stride, padding, dilation)
        if y is None:
            raise RuntimeError("qt_conv2d_bf16 declined a problem its plan took")
        ctx.save_for_backward(xc, wq, wk)
        ctx.conv = (stride, padding, dilation, None if bias is None else tuple(bias.shape), bwd)
        return y

    @staticmethod
    def backward(ctx, gy):
        xc, wq, wk = ctx.saved_tensors
        stride, padding, dilation, bias_shape, bwd = ctx.conv
        need = [ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias_shape is not None and ctx.needs_input_grad[2]]
        in_tree = [need[0] and bwd[0], need[1] and bwd[1], False]
        in_tree[2] = need[2] and (in_tree[0] or in_tree[1] or not (need[0] or need[1]))
        gyc = None
        if any(in_tree):
            gyc = _nhwc_dense(gy)                                       # made NHWC-dense ONCE for every in-tree product
            if gyc.dtype != torch.bfloat16 or gyc.data_ptr() % 16 != 0:
                gyc = gyc.to(torch.bfloat16).clone()
        gx = gw = gb = None
        if in_tree[0]:
            gx = _launch_dgrad(gyc, wk, xc, stride, padding, dilation)
        if in_tree[1]:
            gw = _launch_wgrad(gyc, xc, wk, stride, padding, dilation)
        if in_tree[2]:
            gb = _bias_grad(gyc)
        key = _route_key(xc, wq, stride, padding, dilation, 1)[len("conv2d"):]
        if need[0]:
            CONV_ROUTES.setdefault("conv2d_dgrad" + key, "in_tree_bf16_conv" if gx is not None else "library_conv")
        if need[1]:
            CONV_ROUTES.setdefault("conv2d_wgrad" + key, "in_tree_bf16_conv" if gw is not None else "library_conv")
        mask = [need[0] and gx is None, need[1] and gw is None, need[2] and gb is None]
        if any(mask):
            lx, lw, lb = _library_backward(gy, xc, wq, bias_shape, stride, padding, dilation, mask)
            gx, gw, gb = (lx if mask[0] else gx, lw if mask[1] else gw, lb if mask[2] else gb)
        return (gx, gw, gb, None, None, None, None)


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
        bwd = _backward_routes(mode, n, h, w, cin, cout, kh, kw, stride, pad, dilation)
        return _Conv2dInTree.apply(x, wq, bias, stride, pad, dilation, bwd)
    y = _launch(_nhwc_dense(x), _nhwc_dense(wq), bias, stride, pad, dilation)
    if y is None:
        raise RuntimeError("qt_conv2d_bf16 declined a problem its plan took")
    return y
