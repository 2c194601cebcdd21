"""Native execution of converted per-tensor PT2E graphs (upstream quantize_pt2e.py:323-446).

`convert_pt2e` produces, exactly like upstream,

    xq = quantized_ops.quantize(x, s_x, qmap)        integer / FP8 VALUES held in the model dtype
    y  = aten.linear(xq, W_codes, bias_codes)        (or aten.matmul of two quantized operands)
    out = quantized_ops.dequantize(y, s_x * s_w, out_qmap)

and upstream runs that GEMM in bf16 / fp32 arithmetic on the value tensors.  `fuse_native_gemms` rewrites each such triple
of a DEVICE model into one `quantized_ops.linear_q` / `matmul_q` node that runs the product on the integer / FP8 matrix
cores:

  * int8 x int8: both operands narrowed to int8 codes (weights once, at fusion time), `qt_q8_gemm` -- v_mfma_i32_16x16x64_i8,
    exact int32 accumulation -- with bias, the rounding of the GEMM output to the model dtype, the dequantize multiply and its
    rounding in the epilogue (the rounding points of the three-node sequence are kept);
  * fp8_e4m3 / fp8_e5m2 (per-tensor scaled): operands narrowed to OCP FP8 codes, the in-tree scaled-MFMA GEMM at unit block
    scales (`qt_mx_gemm`; the library GEMM `qt_fp8_gemm` only where that kernel does not take the shape), then the dequantize kernel;
  * int8 convolutions (`quantize -> aten.conv2d -> dequantize`, the ImageNet recipe): one `conv2d_q` node -- the activation to int8
    NHWC codes in one pass (`qt_quantize_codes_nhwc_*`), then `qt_q8_conv2d`, an implicit GEMM on the same instruction with the same
    epilogue, into a channels_last result.  Depthwise layers (groups = Cin = Cout, a multiple of 16) run `qt_q8_dwconv2d` on the same
    codes; 1 x 1, stride 1, unpadded layers over Cin = 16 mod 32 (which the gather kernel declines) run `qt_q8_gemm` on them.
    `fuse_native_gemms(model, split_k=True)` (opt-in: `convert_pt2e(split_k=True)`) marks the gather layers' codes buffers: a marked
    layer launches `qt_q8_conv2d_ws` with the plan's split of K (the same bits) and has a route rule of its own.

`fuse_conv_q_chains` (opt-in: `convert_pt2e(chain_convs=True)`) then hands int8 codes from one such convolution to the next:
`conv2d_q -> aten.relu / hardtanh / clamp -> conv2d_q` becomes two `conv2d_qc` nodes, the first writing the second's codes from its
epilogue (`qt_q8_*_codes`), the activation node gone, the second running no codes pass; bit-identical to the nodes it replaces.

The graph `convert_pt2e` returns is untouched on the CPU (it is pinned node for node to upstream's); fusion is a separate,
idempotent pass that convert_pt2e applies to device models (`native=None` -> automatic, `QT_PT2E_NATIVE=0` turns it off).
Accumulation is exact (int32) where upstream's fp32 / bf16 `aten.linear` rounds, so results agree within the accumulation
bound, not bit for bit.  STATS counts the native launches (tests assert the route was taken).

`fuse_mx_pairs` is the same kind of pass for microscaling graphs: an activation's `calculate_mx_qparam` + `quantize` pair becomes
one `quantize_mx` node (one device pass, bit-identical results).
"""
import ctypes

import torch
from torch.fx import GraphModule

from . import _native, mx_operand, switches
from .fake_quantize import _stream_ptr

__all__ = ["fuse_native_gemms", "fuse_conv_q_chains", "fuse_mx_pairs", "fuse_gwa_linears", "STATS", "GWA_STATS"]

# conv2d_codes_in / conv2d_codes_out: native conv2d_qc launches that took / wrote a code array (counted in their kernel's key as well)
# conv2d_split_k: gather-kernel launches that split K over more than one workgroup per tile (counted in conv2d_int8 as well)
STATS = {"linear_int8": 0, "matmul_int8": 0, "linear_fp8": 0, "matmul_fp8": 0, "conv2d_int8": 0, "conv2d_dw_int8": 0,
         "conv2d_codes_in": 0, "conv2d_codes_out": 0, "conv2d_split_k": 0}
_IDENTITY_DTYPES = (None, "None", "bfloat16", "float32", "float16")
_FP8 = {"fp8_e4m3": torch.float8_e4m3fn, "fp8_e5m2": torch.float8_e5m2}

_lib = torch.library.Library("quantized_ops", "FRAGMENT")
# out_map: the dequantize node's input map (identity for the cases that are fused); kept as an operand so that the CPU / fallback
# formulation below stays the three-node sequence verbatim
_lib.define("linear_q(Tensor input, Tensor scale, Tensor qmap, Tensor weight_codes, Tensor? bias, Tensor out_scale, "
            "Tensor? out_map, str kind) -> Tensor")
_lib.define("matmul_q(Tensor self, Tensor self_scale, Tensor self_qmap, Tensor other, Tensor other_scale, Tensor other_qmap, "
            "bool other_is_kn, Tensor out_scale, Tensor? out_map, str kind) -> Tensor")


def _codes(x, scale, qmap, kind):
    """quantize(x, scale, qmap) narrowed to the format's code type (exact: the values ARE int8 / FP8 values)."""
    v = torch.ops.quantized_ops.quantize(x, scale, None, None, None, qmap)
    return v.to(torch.int8) if kind == "int8" else v.to(_FP8[kind])


def _scale_arg(out_scale, n, dtype):
    s = out_scale.to(dtype).reshape(-1).contiguous()
    if s.numel() not in (1, n):
        raise ValueError(f"dequantize scale of {s.numel()} elements behind a GEMM with {n} output columns")
    return s, int(s.numel() == n and n > 1)


def _q8(a, b, bias, out_scale, out_map, out_shape, batch, M, N, K, a_bs, b_bs, dtype):
    y = torch.empty(out_shape, dtype=dtype, device=a.device)
    fold = int(out_map is not None and dtype == torch.float32)
    s, per_col = _scale_arg(out_scale, N, dtype)
    bias_t = bias.to(dtype).contiguous() if bias is not None else None
    _native.check(_native.lib().qt_q8_gemm(a.data_ptr(), b.data_ptr(), y.data_ptr(), int(dtype == torch.float32),
                                           bias_t.data_ptr() if bias_t is not None else None, s.data_ptr(), per_col, fold, batch, M, N, K,
                                           a_bs, b_bs, _stream_ptr(a)), "qt_q8_gemm")
    return y


_UNIT_E8M0 = {}          # device -> uint8 tensor of 127s (scale 2^0): the block scales of a per-tensor FP8 operand
_UNIT_E8M0_OLD = []      # outgrown buffers stay allocated: a hipGraph captured earlier still reads their addresses
_MX_FMT = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}


def _fp8_codes_gemm(a, w, bias):
    """C = a . w^T (+ bias) on FP8 CODES through the in-tree scaled-MFMA GEMM (qt_mx_gemm, v_mfma_scale_f32_16x16x128_f8f6f4) at unit
    block scales: per-tensor FP8 operands are a block-scaled operand whose every scale is 2^0.  None when the kernel does not take
    the problem (the caller then keeps the library GEMM)."""
    M, K = a.shape
    N = w.shape[0]
    if K % 32 or a.dtype not in _MX_FMT or w.dtype not in _MX_FMT or not a.is_contiguous() or not w.is_contiguous() or a.data_ptr() % 16 or w.data_ptr() % 16:
        return None
    need = max(M, N) * (K // 32)
    ones = _UNIT_E8M0.get(a.device)
    if ones is None or ones.numel() < need:
        if torch.cuda.is_current_stream_capturing():
            return None
        if ones is not None:
            _UNIT_E8M0_OLD.append(ones)
        ones = torch.full((need,), 127, dtype=torch.uint8, device=a.device)
        _UNIT_E8M0[a.device] = ones
    y = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    rc = _native.lib().qt_mx_gemm(a.data_ptr(), ones.data_ptr(), _MX_FMT[a.dtype], w.data_ptr(), ones.data_ptr(), _MX_FMT[w.dtype], y.data_ptr(), 0,
                                  bias.data_ptr() if bias is not None else None, 1, M, N, K, 0, 0, _stream_ptr(a))
    if rc != 0:
        return None
    return y


def _linear_q(input, scale, qmap, weight_codes, bias, out_scale, out_map, kind):
    if input.device.type != "cuda" or input.dtype not in (torch.bfloat16, torch.float32):
        w = weight_codes.to(input.dtype)
        y = torch.nn.functional.linear(torch.ops.quantized_ops.quantize(input, scale, None, None, None, qmap), w, bias)
        return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)
    K, N = input.shape[-1], weight_codes.shape[0]
    a = _codes(input, scale, qmap, kind).reshape(-1, K)
    M = a.shape[0]
    if kind == "int8" and K % 16 == 0 and a.data_ptr() % 16 == 0 and weight_codes.data_ptr() % 16 == 0:
        STATS["linear_int8"] += 1
        return _q8(a, weight_codes, bias, out_scale, out_map, (*input.shape[:-1], N), 1, M, N, K, 0, 0, input.dtype)
    if kind in _FP8 and input.dtype == torch.bfloat16:
        b16 = bias.to(torch.bfloat16).contiguous() if bias is not None else None
        y = _fp8_codes_gemm(a.contiguous(), weight_codes, b16)
        if y is not None:
            STATS["linear_fp8_native"] = STATS.get("linear_fp8_native", 0) + 1
        else:
            from .fused import lt_fp8_gemm
            y = lt_fp8_gemm(a, weight_codes, b16)
        if y is not None:
            STATS["linear_fp8"] += 1
            y = y.reshape(*input.shape[:-1], N)
            return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)
    y = torch.nn.functional.linear(a.to(input.dtype).reshape(input.shape), weight_codes.to(input.dtype), bias)
    return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)


def _matmul_q(self, self_scale, self_qmap, other, other_scale, other_qmap, other_is_kn, out_scale, out_map, kind):
    """self [..., M, K]; other: [..., N, K] (other_is_kn False: the graph multiplied by its transpose) or [..., K, N]."""
    def fallback():
        a = torch.ops.quantized_ops.quantize(self, self_scale, None, None, None, self_qmap)
        b = torch.ops.quantized_ops.quantize(other, other_scale, None, None, None, other_qmap)
        y = torch.matmul(a, b if other_is_kn else b.transpose(-1, -2))
        return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)
    if self.device.type != "cuda" or self.dtype not in (torch.bfloat16, torch.float32) or kind != "int8":
        return fallback()
    if self.dim() < 2 or other.dim() != self.dim() or self.shape[:-2] != other.shape[:-2]:
        return fallback()
    M, K = self.shape[-2], self.shape[-1]
    N = other.shape[-1] if other_is_kn else other.shape[-2]
    if K % 16 != 0 or (other.shape[-2] if other_is_kn else other.shape[-1]) != K:
        return fallback()
    batch = 1
    for d in self.shape[:-2]:
        batch *= d
    a = _codes(self, self_scale, self_qmap, kind).contiguous()
    b = _codes(other, other_scale, other_qmap, kind)
    b = (b.transpose(-1, -2) if other_is_kn else b).contiguous()            # [..., N, K]
    if a.data_ptr() % 16 or b.data_ptr() % 16 or (batch > 1 and (M * K) % 16) or (batch > 1 and (N * K) % 16) or batch > 65535:
        return fallback()
    STATS["matmul_int8"] += 1
    return _q8(a, b, None, out_scale, out_map, (*self.shape[:-2], M, N), batch, M, N, K, M, N, self.dtype)


_lib.impl("linear_q", _linear_q, "CompositeExplicitAutograd")
_lib.impl("matmul_q", _matmul_q, "CompositeExplicitAutograd")


# ---- quantize -> aten.conv2d -> dequantize: conv2d_q (csrc/qt_mx_conv.hip qt_q8_conv2d, csrc/qt_elementwise.hip qt_quantize_codes_nhwc_*) ----
# weight_codes is int8 [Cout, kh, kw, Cin]: its shape carries the filter geometry and, flattened, it is the kernel's [Cout][kh kw Cin]
# operand.  The activation becomes int8 NHWC codes in one pass (no value tensor), the implicit GEMM accumulates in int32 and its
# epilogue keeps the rounding points of the three nodes.  Everything the kernels do not take runs those three nodes verbatim.
_lib.define("conv2d_q(Tensor input, Tensor scale, Tensor qmap, Tensor weight_codes, Tensor? bias, int[2] stride, int[2] padding, "
            "int[2] dilation, int groups, Tensor out_scale, Tensor? out_map, str kind) -> Tensor")

CONV_Q_REASONS = {}            # why a device call of conv2d_q ran the three-node sequence -> count
_APPLY_CONV_Q_RULE = True      # tools/exp_conv_q.py clears it to time the route the rule below declines
_CONV_Q_MAX_K = 1 << 17


def _conv_q_route_takes(m, cout, cin, kh, kw):
    """The committed rule, a fixed function of the shape (never a timing): m = N Ho Wo output pixels, cout and cin channels, the
    filter.  From profiles/conv2d_q.txt (ResNet-50's thirteen body layers at batch 32 and five smaller problems, bf16; the graph's
    quantize + aten.conv2d + dequantize against conv2d_q with the codes pass inside the call, NCHW-contiguous and channels_last
    input, eager calls and hipGraph replays).  A class is listed only where the native median beat the graph's median by more than
    the graph's own min-max spread on every row, layout and mode; t = the kernel's 128 x 128 output tiles:
      * filters larger than 1 x 1 with t >= 52: all five rows clear (3 x 3 at 64 - 512 channels, 7 x 7 over 32; 1.24 - 3.4 x);
      * 1 x 1 with Cout >= Cin and t >= 208: all five rows clear (1.14 - 2.1 x);
      * 1 x 1 with Cout < Cin: two of the four rows clear (256 -> 64 at 56 x 56: 1.44 - 3.0 x; 512 -> 128 at 28 x 28: 1.05 x from
        NCHW input) and two lose -- a long contraction over few column tiles, no split of K: replayed from NCHW input 0.70 x
        (2048 -> 512), 0.87 x (1024 -> 256) -- so the class is not listed;
      * a few tiles (batch 4: t <= 8): none of the four rows clears (0.64 - 1.00 x replayed from NCHW input)."""
    tiles = -(-m // 128) * -(-cout // 128)
    if kh * kw > 1:
        return tiles >= 52
    return cout >= cin and tiles >= 208


_SPLIT_PROFILE = "profiles/conv2d_q_splitk.txt"


def mark_split_k(weight_codes):
    """Opts a gather layer's int8 codes buffer into the split of K (fuse_native_gemms(split_k=True) does this for every gather
    layer).  The mark is an attribute of the tensor object, like _qt_conv_values: a copy or a move of the buffer loses it, and the
    layer then routes exactly as an unmarked one."""
    weight_codes._qt_split_k = True
    return weight_codes


def _split_k_marked(weight_codes):
    return getattr(weight_codes, "_qt_split_k", False) is True


def _conv_q_split_route_takes(m, cout, cin, kh, kw):
    """The committed rule for gather layers whose codes buffer carries the split-K mark, consulted where _conv_q_route_takes says
    no; a fixed function of the shape (never a timing).  From profiles/conv2d_q_splitk.txt (seventeen rows, bf16: ResNet-50's four
    reducing 1 x 1 layers and 512 -> 512 3 x 3 at 7 x 7, batch 32; the four batch-4 problems of profiles/conv2d_q.txt; MobileNetV2's
    eight projecting layers over Cin % 32 == 0, batch 32; the method and the bar of profiles/conv2d_q.txt, judged at the split
    qt_q8_conv2d_plan chooses; t = 128 x 128 output tiles, nk = k tiles of 128).  One class is listed:
      * filters larger than 1 x 1 with nk >= 36 and t >= 8: both measured rows clear -- 4 x 512 -> 512 3 x 3 at 7 x 7 (t = 8, S = 8:
        replayed 45.4 -> 42.5 us from NCHW input, 49.9 -> 38.3 from channels_last, where the unsplit kernel takes 71.3 / 66.7) and
        the same layer at batch 32 (t = 52, S = 4: 93.6 -> 46.9 / 99.2 -> 42.6 against 72.5 / 67.4 unsplit; _conv_q_route_takes
        lists it already).
    Not listed, because a row of the class loses: reducing 1 x 1 layers -- the split shortens the launch (2048 -> 512: 37.6 -> 30.4 us
    alone) but the call with its codes pass still loses from NCHW input (36.4 -> 45.3 us; 1024 -> 256: 40.0 -> 46.3); MobileNetV2's
    projecting layers (960 -> 160 clears at S = 4 by 0.8 us; 960 -> 320, 576 -> 96, 576 -> 160 and 384 -> 96 lose replayed from NCHW input:
    no class separates them but the rows themselves); the three small batch-4 problems (nk <= 5: 0.79 - 0.95 x)."""
    tiles, nk = -(-m // 128) * -(-cout // 128), -(-kh * kw * cin // 128)
    return kh * kw > 1 and nk >= 36 and tiles >= 8


_DW_PROFILE = "profiles/conv2d_q_depthwise.txt"
_CONV_Q_DW_MAX_TAPS = 1023


def _conv_q_dw_route_takes(m, c, kh, kw, sh, sw):
    """The committed rule for depthwise calls (groups = Cin = Cout = c), a fixed function of the shape (never a timing): m = N Ho Wo
    output pixels, the filter, the strides.  From profiles/conv2d_q_depthwise.txt (MobileNetV2's ten depthwise shapes at batch 32, a
    5 x 5 layer over 240 channels, two batch-4 problems; bf16; the method and the bar of profiles/conv2d_q.txt): all thirteen rows
    clear the bar -- replayed 1.5 - 3.8 x from NCHW input and 2.7 - 5.2 x from channels_last at batch 32, 1.10 x / 1.85 x on the
    smallest problem (4 x 576 x 14 x 14: 20.6 -> 18.7 us against a spread of 0.1).  The class is what was measured: filters of at most
    25 taps, strides of at most 2, at least as many output elements as that smallest problem.  Anything else (a 7 x 7 filter, stride
    3, a smaller problem) was not measured and stays with the graph."""
    return kh * kw <= 25 and max(sh, sw) <= 2 and m * c >= _DW_MIN_OUTPUTS


_DW_MIN_OUTPUTS = 4 * 14 * 14 * 576
_PW16_MIN_PIXELS, _PW16_MAX_CIN = 32 * 28 * 28, 144


def _conv_q_pw16_route_takes(m, cout, cin):
    """The committed rule for 1 x 1, stride 1, unpadded calls over Cin = 16 mod 32 channels (codes pass + qt_q8_gemm), a fixed function
    of the shape.  From the three pointwise rows of profiles/conv2d_q_depthwise.txt (16 -> 96 at 112 x 112, 144 -> 24 at 56 x 56,
    144 -> 32 at 28 x 28, batch 32): all clear the bar, replayed 1.14 - 1.45 x from NCHW input and 1.50 - 3.2 x from channels_last.  The
    class is what was measured: at least 32 x 28 x 28 output pixels and Cin of at most 144; a longer contraction over fewer pixels
    is the shape on which the gather kernel's reducing 1 x 1 layers lose, and stays with the graph."""
    return m >= _PW16_MIN_PIXELS and cin <= _PW16_MAX_CIN


def _conv_q_route(input, weight_codes, stride, padding, groups):
    """Which kernel a 4-D call would run on: "depthwise" (qt_q8_dwconv2d: groups = Cin = Cout, one filter per channel), "pointwise"
    (qt_q8_gemm: a 1 x 1, stride 1, unpadded convolution over NHWC codes is the GEMM [N H W][Cin] x [Cout][Cin]^T, taken there for the
    Cin = 16 mod 32 that the gather kernel declines), "gather" (qt_q8_conv2d), or None for any other grouped call."""
    cin = input.shape[1]
    cout, kh, kw, wcin = weight_codes.shape
    if groups != 1:
        return "depthwise" if groups == cin == cout and wcin == 1 else None
    if kh == kw == 1 and list(stride) == [1, 1] and list(padding) == [0, 0] and wcin == cin and cin >= 16 and cin % 32 == 16:
        return "pointwise"
    return "gather"


def _conv_out_hw(h, w, kh, kw, stride, padding, dilation):
    ho = (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1 if stride[0] > 0 else 0
    wo = (w + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1 if stride[1] > 0 else 0
    return ho, wo


def _conv_q_decline(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, kind, on_device=None):
    """Why the kernels do not take this call (a string), or None when they do.  `on_device` overrides the device test, so that the
    rest of the predicate can be exercised with host tensors."""
    if not (input.device.type == "cuda" if on_device is None else on_device):
        return "not a device tensor"
    if kind != "int8" or weight_codes.dtype != torch.int8:
        return f"kind {kind}, weight codes {weight_codes.dtype}"
    if input.dtype not in (torch.bfloat16, torch.float32):
        return f"model dtype {input.dtype}"
    if input.dim() != 4 or weight_codes.dim() != 4 or input.numel() == 0 or weight_codes.numel() == 0:
        return f"input {tuple(input.shape)}, weight codes {tuple(weight_codes.shape)}"
    route = _conv_q_route(input, weight_codes, stride, padding, groups)
    if route is None:
        return f"groups {groups}"
    n, cin, h, w = input.shape
    cout, kh, kw, wcin = weight_codes.shape
    if route == "depthwise":
        if cin < 16 or cin % 16:
            return f"depthwise C = {cin}: not a multiple of 16"
        if kh * kw > _CONV_Q_DW_MAX_TAPS:
            return f"depthwise kh kw = {kh * kw} > 1023"
    else:
        if route == "gather" and (wcin != cin or cin < 32 or cin % 32):
            return f"Cin = {cin} / {wcin}: not a multiple of 32"
        if kh * kw * cin >= _CONV_Q_MAX_K:
            return f"kh kw Cin = {kh * kw * cin} >= 2^17: the int32 sum could wrap"
    if qmap.dtype != torch.bfloat16 or qmap.numel() != 65536:
        return f"value map of {qmap.numel()} {qmap.dtype} entries"
    if scale.numel() != 1 or scale.dtype != input.dtype:
        return f"activation scale of {scale.numel()} elements, {scale.dtype}"
    if out_scale.numel() not in (1, cout):
        return f"dequantize scale of {out_scale.numel()} elements behind {cout} output channels"
    if bias is not None and bias.numel() != cout:
        return f"bias of {bias.numel()} elements"
    ho, wo = _conv_out_hw(h, w, kh, kw, stride, padding, dilation)
    if ho < 1 or wo < 1:
        return f"empty output {ho} x {wo}"
    if input.data_ptr() % 16 or weight_codes.data_ptr() % 16 or not weight_codes.is_contiguous() or qmap.data_ptr() % 2 \
            or not qmap.is_contiguous():
        return "misaligned operand"
    if _APPLY_CONV_Q_RULE:
        if route == "depthwise" and not _conv_q_dw_route_takes(n * ho * wo, cin, kh, kw, stride[0], stride[1]):
            return f"depthwise route rule: {_DW_PROFILE}"
        if route == "pointwise" and not _conv_q_pw16_route_takes(n * ho * wo, cout, cin):
            return f"pointwise route rule: {_DW_PROFILE}"
        if route == "gather" and not _conv_q_route_takes(n * ho * wo, cout, cin, kh, kw):
            if not _split_k_marked(weight_codes):
                return "route rule: profiles/conv2d_q.txt"
            if not _conv_q_split_route_takes(n * ho * wo, cout, cin, kh, kw):
                return f"split-K route rule: {_SPLIT_PROFILE}"
    return None


def _aligned16(t):
    return t.clone() if t.data_ptr() % 16 else t


def _conv_weight_values(weight_codes, dtype):
    """[Cout, Cin, kh, kw] values of the codes in the model dtype, as the unfused graph stored them.  The pass leaves the layer's own
    parameter here (no copy: a fused layer holds its parameter as before plus 1 B per weight of codes); a codes tensor that lost it
    (moved or copied since, or built by hand) gets the values rebuilt once and kept, unless the stream is capturing (a tensor
    allocated during a capture belongs to that graph's pool)."""
    cache = getattr(weight_codes, "_qt_conv_values", None)
    if cache is not None and cache.dtype == dtype and cache.device == weight_codes.device:
        return cache
    w = weight_codes.permute(0, 3, 1, 2).to(dtype).contiguous()
    if not (weight_codes.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
        weight_codes._qt_conv_values = w
    return w


def _conv2d_q_unfused(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map):
    xq = torch.ops.quantized_ops.quantize(input, scale, None, None, None, qmap)
    y = torch.nn.functional.conv2d(xq, _conv_weight_values(weight_codes, input.dtype), bias, tuple(stride), tuple(padding),
                                   tuple(dilation), groups)
    return torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)


def conv_codes_nhwc(input, scale, qmap):
    """int8 codes [N H W, C] of quantize(input, scale, qmap) in one pass (qt_quantize_codes_nhwc_*), or None when declined."""
    from .decomposed import _lut_format, _scalar_like
    from .mx_conv import _nhwc_strides
    n, c, h, w = input.shape
    xs = _nhwc_strides(input)
    if xs is None:
        input, xs = input.contiguous(), (c * h * w, 1, h * w)
    codes = torch.empty((n * h * w, c), dtype=torch.int8, device=input.device)
    s = _scalar_like(scale, input)
    fmt = _lut_format()
    L = _native.lib()
    fn = L.qt_quantize_codes_nhwc_bf16 if input.dtype == torch.bfloat16 else L.qt_quantize_codes_nhwc_f32
    rc = fn(input.data_ptr(), codes.data_ptr(), n, h * w, c, *xs, ctypes.byref(fmt), qmap.data_ptr(), s.data_ptr(), _stream_ptr(input))
    if _native.declined(rc):
        return None
    _native.check(rc, "qt_quantize_codes_nhwc")
    return codes


class _Operand:
    """What _conv_q_route and _conv_q_decline read of an operand, for one that is not there as a value tensor: the activation of a
    call that receives codes (their geometry under the model dtype), the scale and map such a call no longer has, a graph node known
    by its shape alone.  Dense and aligned unless `ptr` says otherwise."""

    def __init__(self, shape, dtype, device, ptr=0):
        self.shape, self.dtype, self.device, self._ptr = torch.Size(shape), dtype, torch.device(device), ptr

    def dim(self):
        return len(self.shape)

    def numel(self):
        return self.shape.numel()

    def data_ptr(self):
        return self._ptr

    def is_contiguous(self):
        return True


def _conv_q_launch(codes, shape, dtype, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map, tail=None):
    """One native launch on the NHWC codes [N H W, Cin] of an activation of logical `shape`, on the kernel _conv_q_route names.
    tail None: the value tensor [N, Cout, Ho, Wo] in `dtype`, channels_last (qt_q8_dwconv2d / qt_q8_gemm / qt_q8_conv2d).
    tail (act, lo, hi, next_scale, next_qmap): the consumer's int8 codes in the same layout (the *_codes siblings).
    -> (result, None), or (None, why) when the entry point declines the shape."""
    n, cin, h, w = shape
    cout, kh, kw, _ = weight_codes.shape
    ho, wo = _conv_out_hw(h, w, kh, kw, stride, padding, dilation)
    out = torch.empty((n, cout, ho, wo), dtype=dtype if tail is None else torch.int8, device=codes.device, memory_format=torch.channels_last)
    s, per_col = _scale_arg(out_scale, cout, dtype)
    s = _aligned16(s)
    b = _aligned16(bias.to(dtype).contiguous()) if bias is not None else None
    fold = int(out_map is not None and dtype == torch.float32)
    route = _conv_q_route(_Operand(shape, dtype, codes.device), weight_codes, stride, padding, groups)
    L = _native.lib()
    stream = _stream_ptr(codes)
    head = (codes.data_ptr(), weight_codes.data_ptr(), out.data_ptr(), int(dtype == torch.float32),
            b.data_ptr() if b is not None else None, s.data_ptr(), per_col, fold)
    geometry = (kh, kw, stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1])
    last, sfx, split = (stream,), "", 1
    if tail is not None:
        act, lo, hi, next_scale, next_qmap = tail
        last, sfx = (int(act), float(lo), float(hi), next_scale.data_ptr(), next_qmap.data_ptr(), stream), "_codes"
    if route == "depthwise":                     # weight_codes [C, kh, kw, 1] is the kernel's [C][kh][kw] as stored
        entry, key, rc = "qt_q8_dwconv2d" + sfx, "conv2d_dw_int8", getattr(L, "qt_q8_dwconv2d" + sfx)(*head, n, h, w, cin, *geometry, *last)
    elif route == "pointwise":                   # the channels_last result is the row-major [N Ho Wo][Cout] of the GEMM
        entry, key, rc = "qt_q8_gemm" + sfx, "conv2d_int8", getattr(L, "qt_q8_gemm" + sfx)(*head, 1, n * h * w, cout, cin, 0, 0, *last)
    elif _split_k_marked(weight_codes):          # the plan's split (1: the unsplit kernel, no workspace) through the *_ws sibling
        from .fused import splitk_scratch
        split, wbytes, ntick = _native.q8_conv_plan(n * ho * wo, cout, kh * kw * cin)
        ws, tickets = splitk_scratch("conv_q", wbytes, ntick, codes.device) if split > 1 else (None, None)
        scratch = (split, ws.data_ptr() if split > 1 else None, ws.numel() * 4 if split > 1 else 0,
                   tickets.data_ptr() if split > 1 else None, tickets.numel() if split > 1 else 0)
        entry, key = "qt_q8_conv2d" + sfx + "_ws", "conv2d_int8"
        rc = getattr(L, entry)(*head, n, h, w, cin, cout, *geometry, *last[:-1], *scratch, stream)
    else:
        entry, key, rc = "qt_q8_conv2d" + sfx, "conv2d_int8", getattr(L, "qt_q8_conv2d" + sfx)(*head, n, h, w, cin, cout, *geometry, *last)
    if _native.declined(rc):
        return None, f"{entry} declined the shape (code {rc})"
    _native.check(rc, entry)
    STATS[key] += 1
    STATS["conv2d_split_k"] += int(split > 1)
    return out, None


def _conv2d_q(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map, kind):
    stride, padding, dilation = [int(v) for v in stride], [int(v) for v in padding], [int(v) for v in dilation]
    why = _conv_q_decline(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, kind)
    if why is None:
        codes = conv_codes_nhwc(input, scale, qmap)
        if codes is None:
            why = "qt_quantize_codes_nhwc declined"
        else:
            out, why = _conv_q_launch(codes, input.shape, input.dtype, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map)
            if why is None:
                return out
    if input.device.type == "cuda":
        CONV_Q_REASONS[why] = CONV_Q_REASONS.get(why, 0) + 1
    return _conv2d_q_unfused(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map)


def _conv2d_q_meta(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map, kind):
    ho, wo = _conv_out_hw(input.shape[2], input.shape[3], weight_codes.shape[1], weight_codes.shape[2], list(stride), list(padding),
                          list(dilation))
    return input.new_empty((input.shape[0], weight_codes.shape[0], ho, wo))


_lib.impl("conv2d_q", _conv2d_q, "CompositeExplicitAutograd")
_lib.impl("conv2d_q", _conv2d_q_meta, "Meta")


# ---- chained converted convolutions: codes in, codes out ------------------------------------------------------------------------
# Between two conv2d_q nodes the converted graph runs
#     y = conv2d_q(...)                       the kernel rounds its int32 sum to the model dtype and writes it
#     a = aten.relu / hardtanh / clamp(y)     read and written again
#     conv2d_q(a, s_next, qmap_next, ...)     whose codes pass reads it a third time to write 1 B per element
# fuse_conv_q_chains makes the producer a conv2d_qc that writes s_next / qmap_next codes from its epilogue (qt_q8_*_codes: the
# activation and the consumer's quantize applied to the element in its register), erases the activation node, and makes each
# consumer a conv2d_qc that takes the code array as its input (scale = qmap = None: no codes pass).  conv2d_qc is conv2d_q plus
#     scale, qmap None      `input` is int8 [N, C, H, W] codes, channels_last; the model dtype is out_scale's
#     next_scale, next_qmap the result is the int8 [N, Cout, Ho, Wo] codes quantize(act(y), next_scale, next_qmap), channels_last
#     act_min, act_max      the clamp in front of that quantize (relu: 0, None); only with codes out
# Eligibility is conv2d_q's (_conv_q_decline and the committed route rules, measured with the codes pass inside the call: a call
# that receives codes is only cheaper); every decline runs the value-tensor nodes and gives the same bits.
_lib.define("conv2d_qc(Tensor input, Tensor? scale, Tensor? qmap, Tensor weight_codes, Tensor? bias, int[2] stride, int[2] padding, "
            "int[2] dilation, int groups, Tensor out_scale, Tensor? out_map, str kind, float? act_min, float? act_max, "
            "Tensor? next_scale, Tensor? next_qmap) -> Tensor")


def _narrow_codes(v):
    """Values of a quantize node -> int8 by the rule of the device's code_of: NaN -> 0, saturate to [-128, 127], truncate."""
    return torch.nan_to_num(v.float(), nan=0.0, posinf=127.0, neginf=-128.0).clamp(-128.0, 127.0).to(torch.int8)


def _codes_of_values(y, act_min, act_max, next_scale, next_qmap):
    """The graph's own tail on a value tensor: the activation, then the consumer's quantize as int8 [N, C, H, W], channels_last."""
    if act_min is not None or act_max is not None:
        y = torch.clamp(y, min=act_min, max=act_max)
    n, c, h, w = y.shape
    codes = None
    if y.device.type == "cuda" and y.dtype in (torch.bfloat16, torch.float32) and c % 16 == 0 and y.numel() and next_scale.numel() == 1 \
            and next_scale.dtype == y.dtype and next_qmap.dtype == torch.bfloat16 and next_qmap.numel() == 65536:
        codes = conv_codes_nhwc(y, next_scale, next_qmap)
    if codes is not None:
        return codes.view(n, h, w, c).permute(0, 3, 1, 2)
    return _narrow_codes(torch.ops.quantized_ops.quantize(y, next_scale, None, None, None, next_qmap)).contiguous(memory_format=torch.channels_last)


def _conv2d_qc(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map, kind, act_min, act_max,
               next_scale, next_qmap):
    codes_in, codes_out = scale is None, next_scale is not None
    if codes_in and (qmap is not None or input.dtype != torch.int8 or input.dim() != 4):
        raise ValueError("conv2d_qc without a scale takes int8 [N, C, H, W] codes and no map")
    if not codes_in and qmap is None:
        raise ValueError("conv2d_qc with a scale needs the value map")
    if codes_out and next_qmap is None:
        raise ValueError("conv2d_qc with next_scale needs next_qmap")
    if not codes_out and (act_min is not None or act_max is not None or next_qmap is not None):
        raise ValueError("conv2d_qc: the activation bounds and next_qmap go with next_scale (codes out)")
    if act_min is not None and act_max is not None and not act_min <= act_max:
        raise ValueError(f"conv2d_qc: clamp bounds {act_min} > {act_max}")
    args = (weight_codes, bias, stride, padding, dilation, groups, out_scale)
    if not codes_in and not codes_out:
        return torch.ops.quantized_ops.conv2d_q(input, scale, qmap, *args, out_map, kind)
    stride, padding, dilation = [int(v) for v in stride], [int(v) for v in padding], [int(v) for v in dilation]
    args = (weight_codes, bias, stride, padding, dilation, groups, out_scale)
    dtype = out_scale.dtype if codes_in else input.dtype
    device = input.device.type == "cuda"

    def note(why):
        if device:
            CONV_Q_REASONS[why] = CONV_Q_REASONS.get(why, 0) + 1

    if codes_in:
        if not input.permute(0, 2, 3, 1).is_contiguous():
            input = input.contiguous(memory_format=torch.channels_last)
        why = _conv_q_decline(_Operand(input.shape, dtype, input.device, input.data_ptr()), _Operand((1,), dtype, input.device),
                              _Operand((65536,), torch.bfloat16, input.device), *args, kind)
    else:
        why = _conv_q_decline(input, scale, qmap, *args, kind)
    tail = None
    if codes_out:
        tail = (int(act_min is not None or act_max is not None), float("-inf") if act_min is None else act_min,
                float("inf") if act_max is None else act_max, next_scale, next_qmap)
    why_out = None
    if why is None and codes_out:
        cout = weight_codes.shape[0]
        if cout % 16:
            why_out = f"codes out: Cout = {cout} is not a multiple of 16"
        elif next_scale.numel() != 1 or next_scale.dtype != dtype or next_qmap.dtype != torch.bfloat16 or next_qmap.numel() != 65536 \
                or not next_qmap.is_contiguous():
            why_out = f"codes out: scale of {next_scale.numel()} {next_scale.dtype}, map of {next_qmap.numel()} {next_qmap.dtype} entries"
    y = None
    if why is None:
        n, c, h, w = input.shape
        codes = input.permute(0, 2, 3, 1).reshape(n * h * w, c) if codes_in else None
        if codes_out and why_out is None:
            if not codes_in:
                codes = conv_codes_nhwc(input, scale, qmap)
            if codes is None:
                why_out = "qt_quantize_codes_nhwc declined"
            else:
                out, why_out = _conv_q_launch(codes, input.shape, dtype, *args, out_map, tail)
                if why_out is None:
                    STATS["conv2d_codes_out"] += 1
                    STATS["conv2d_codes_in"] += int(codes_in)
                    return out
        if codes_in:                                    # values out, or the value tensor the graph's own tail turns into codes
            y, why = _conv_q_launch(codes, input.shape, dtype, *args, out_map)
            if why is None:
                STATS["conv2d_codes_in"] += 1
        if why is None and why_out is not None:
            note(why_out)
    if y is None and codes_in:
        # the values quantize would have produced, dense in NCHW order as quantize returns them (a library convolution need not sum
        # in the same order for two layouts of one tensor), through the graph's own nodes
        note(why)
        w_values = _conv_weight_values(weight_codes, dtype)
        y = torch.nn.functional.conv2d(input.to(dtype).contiguous(), w_values, bias, tuple(stride), tuple(padding), tuple(dilation), groups)
        y = torch.ops.quantized_ops.dequantize(y, out_scale, None, None, None, out_map)
    elif y is None:                                     # conv2d_q on whichever route it takes; it records its own decline
        y = torch.ops.quantized_ops.conv2d_q(input, scale, qmap, *args, out_map, kind)
    if not codes_out:
        return y
    return _codes_of_values(y, act_min, act_max, next_scale, next_qmap)


def _conv2d_qc_meta(input, scale, qmap, weight_codes, bias, stride, padding, dilation, groups, out_scale, out_map, kind, act_min, act_max,
                    next_scale, next_qmap):
    ho, wo = _conv_out_hw(input.shape[2], input.shape[3], weight_codes.shape[1], weight_codes.shape[2], list(stride), list(padding),
                          list(dilation))
    dtype = torch.int8 if next_scale is not None else (out_scale.dtype if scale is None else input.dtype)
    return input.new_empty((input.shape[0], weight_codes.shape[0], ho, wo), dtype=dtype)


_lib.impl("conv2d_qc", _conv2d_qc, "CompositeExplicitAutograd")
_lib.impl("conv2d_qc", _conv2d_qc_meta, "Meta")


def _is(node, target):
    return node is not None and getattr(node, "op", None) == "call_function" and node.target == target


def _per_tensor_quantize(node):
    """`quantize(x, scale, None, None, None, qmap)` with a per-tensor scale -> (x, scale node, qmap node, dtype) or None."""
    Q = torch.ops.quantized_ops.quantize.default
    if not _is(node, Q) or len(node.args) < 6 or node.kwargs:
        return None
    x, s, zp, axes, bs, qmap = node.args[:6]
    if zp is not None or axes is not None or bs is not None or qmap is None or len(node.args) > 6 and node.args[6] is not None:
        return None
    return x, s, qmap, str(node.meta.get("dtype"))


def _sole_dequantize(model, node, dtype):
    """The `dequantize(gemm, scale, None, None, None, input_qmap)` node behind a GEMM or convolution (quantize_pt2e.py:409-413: the GEMM
    output is first rounded to the accelerator's output format through `input_qmap`, then multiplied by s_x * s_w).  Fusable
    when that map is the identity for the model dtype (output_dtype None, or bfloat16 in a bf16 model).
    Returns (dequantize node, scale node, input map node or None) or None."""
    DQ = torch.ops.quantized_ops.dequantize.default
    users = list(node.users.keys())
    if len(users) != 1 or not _is(users[0], DQ):
        return None
    dq = users[0]
    a = list(dq.args) + [None] * (7 - len(dq.args))
    if a[0] is not node or a[2] is not None or a[3] is not None or a[4] is not None or a[6] is not None or dq.kwargs:
        return None
    if a[5] is not None:
        try:
            tag = mx_operand.map_name(model.get_buffer(a[5].target))
        except AttributeError:
            return None
        if not (tag in ("None", "float32") or (tag == "bfloat16" and dtype == torch.bfloat16)):
            return None
    return dq, a[1], a[5]


def fuse_native_gemms(model: GraphModule, split_k: bool = False) -> int:
    """Rewrites quantize -> aten.linear / aten.matmul -> dequantize triples whose operands are int8 (or FP8) codes into
    linear_q / matmul_q nodes, and quantize -> aten.conv2d -> dequantize triples on int8 codes (static geometry; Cin a multiple
    of 32, or depthwise over a multiple of 16 channels, or 1 x 1 / stride 1 / unpadded over Cin = 16 mod 32) into conv2d_q nodes.  Returns the number of fused GEMMs and convolutions; leaves everything else as it is.
    split_k=True marks the int8 codes buffer of every gather layer (groups = 1, Cin a multiple of 32) with mark_split_k: such a layer
    launches qt_q8_conv2d_ws / qt_q8_conv2d_codes_ws with the plan's split and is routed by _conv_q_split_route_takes where
    _conv_q_route_takes declines it.  The graph itself is the same either way."""
    graph = model.graph
    fused = 0
    for node in list(graph.nodes):
        if _is(node, torch.ops.aten.linear.default):
            q = _per_tensor_quantize(node.args[0])
            w = node.args[1]
            if q is None or w.op != "get_attr":
                continue
            kind = q[3].split(",")[0]
            if kind not in ("int8", "fp8_e4m3", "fp8_e5m2") or str(w.meta.get("dtype", "")).split(",")[0] != kind:
                continue
            param = model.get_parameter(w.target) if w.target in dict(model.named_parameters()) else model.get_buffer(w.target)
            tail = _sole_dequantize(model, node, param.dtype)
            if tail is None:
                continue
            dq, s_out, m_out = tail
            codes = param.detach().to(torch.int8) if kind == "int8" else param.detach().to(_FP8[kind])
            if not torch.equal(codes.to(param.dtype), param.detach()):
                continue                                     # not exactly representable: keep the value-tensor GEMM
            name = str(w.target).replace(".", "_") + "_codes"
            i = 0
            while hasattr(model, name):
                i += 1
                name = f"{str(w.target).replace('.', '_')}_codes_{i}"
            model.register_buffer(name, codes.contiguous(), persistent=False)
            bias = node.args[2] if len(node.args) > 2 else None
            with graph.inserting_before(dq):
                c_node = graph.create_node("get_attr", name)
                new = graph.call_function(torch.ops.quantized_ops.linear_q.default,
                                          (q[0], q[1], q[2], c_node, bias, s_out, m_out, kind))
            new.meta = dict(dq.meta)
            dq.replace_all_uses_with(new)
            graph.erase_node(dq)
            graph.erase_node(node)
            fused += 1
        elif _is(node, torch.ops.aten.matmul.default):
            qa, qb = _per_tensor_quantize(node.args[0]), _per_tensor_quantize(node.args[1])
            if qa is None or qb is None:
                continue
            kind = qa[3].split(",")[0]
            if kind != "int8" or qb[3].split(",")[0] != kind:
                continue
            first = next(iter(model.parameters()), None)
            if first is None:
                first = next(iter(model.buffers()), None)
            if first is None:
                continue                                     # a graph without parameters or buffers: nothing says what dtype it runs in
            tail = _sole_dequantize(model, node, first.dtype)
            if tail is None:
                continue
            dq, s_out, m_out = tail
            other, kn = qb[0], True
            if _is(other, torch.ops.aten.transpose.int) and sorted(int(a) for a in other.args[1:3]) == [-2, -1]:
                other, kn = other.args[0], False             # quantize(x^T) = quantize(x)^T: take the [N, K] operand as stored
            with graph.inserting_before(dq):
                new = graph.call_function(torch.ops.quantized_ops.matmul_q.default,
                                          (qa[0], qa[1], qa[2], other, qb[1], qb[2], kn, s_out, m_out, kind))
            new.meta = dict(dq.meta)
            dq.replace_all_uses_with(new)
            graph.erase_node(dq)
            graph.erase_node(node)
            fused += 1
        elif _is(node, torch.ops.aten.conv2d.default):
            a = _conv_args(node)
            if a is None:
                continue
            x_q, w, bias, stride, padding, dilation, groups = a
            q = _per_tensor_quantize(x_q)
            if q is None or getattr(w, "op", None) != "get_attr":
                continue
            if q[3].split(",")[0] != "int8" or str(w.meta.get("dtype", "")).split(",")[0] != "int8":
                continue
            param = model.get_parameter(w.target) if w.target in dict(model.named_parameters()) else model.get_buffer(w.target)
            if param.dim() != 4:
                continue
            cout_w, cin_w, kh_w, kw_w = param.shape
            gather = cin_w >= 32 and cin_w % 32 == 0
            depthwise = groups > 1 and groups == cout_w and cin_w == 1 and groups % 16 == 0
            pointwise = (groups == 1 and kh_w == kw_w == 1 and stride == [1, 1] and padding == [0, 0] and cin_w >= 16
                         and cin_w % 32 == 16)
            if not (gather or depthwise or pointwise):
                continue                                     # channels no kernel ever takes (a stem, Cin = 24, any other grouping): the node stays
            tail = _sole_dequantize(model, node, param.dtype)
            if tail is None:
                continue
            dq, s_out, m_out = tail
            codes = param.detach().to(torch.int8)
            if not torch.equal(codes.to(param.dtype), param.detach()):
                continue                                     # not exactly representable: keep the value-tensor convolution
            name = str(w.target).replace(".", "_") + "_codes"
            i = 0
            while hasattr(model, name):
                i += 1
                name = f"{str(w.target).replace('.', '_')}_codes_{i}"
            model.register_buffer(name, codes.permute(0, 2, 3, 1).contiguous(), persistent=False)       # [Cout, kh, kw, Cin]
            if param.is_contiguous():
                # a call the kernels decline convolves the values the graph stored: the parameter itself, not a third copy
                getattr(model, name)._qt_conv_values = param.detach()
            if split_k and gather and groups == 1:
                mark_split_k(getattr(model, name))
            with graph.inserting_before(dq):
                c_node = graph.create_node("get_attr", name)
                new = graph.call_function(torch.ops.quantized_ops.conv2d_q.default,
                                          (q[0], q[1], q[2], c_node, bias, stride, padding, dilation, groups, s_out, m_out, "int8"))
            c_node.meta["dtype"] = w.meta.get("dtype")
            new.meta = dict(dq.meta)
            dq.replace_all_uses_with(new)
            graph.erase_node(dq)
            graph.erase_node(node)
            fused += 1
    if fused:
        graph.eliminate_dead_code(is_impure_node=lambda n: n.op in {"placeholder", "output"})
        graph.lint()
        model.recompile()
    return fused


def _conv_args(node):
    """(input, weight, bias, stride, padding, dilation, groups) of an aten.conv2d node with the defaults filled in and the geometry as
    two-element int lists; None when an argument is not static (a graph node, a string padding, a symbolic size)."""
    names = ("input", "weight", "bias", "stride", "padding", "dilation", "groups")
    vals = dict(zip(names, (None, None, None, 1, 0, 1, 1)))
    if len(node.args) > len(names) or any(k not in names for k in node.kwargs):
        return None
    vals.update(zip(names, node.args))
    vals.update(node.kwargs)
    out = [vals["input"], vals["weight"], vals["bias"]]
    for k in ("stride", "padding", "dilation"):
        v = vals[k]
        v = [v, v] if isinstance(v, int) and not isinstance(v, bool) else v
        if not isinstance(v, (list, tuple)) or len(v) not in (1, 2) or any(not isinstance(e, int) or isinstance(e, bool) for e in v):
            return None
        out.append([int(e) for e in v] * (2 if len(v) == 1 else 1))
    if not isinstance(vals["groups"], int) or isinstance(vals["groups"], bool):
        return None
    if vals["bias"] is not None and not isinstance(vals["bias"], torch.fx.Node):
        return None
    return (*out, vals["groups"])


def _static_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _chain_activation(node):
    """(lo, hi) of an activation the *_codes epilogues apply -- aten.relu(_), hardtanh(_), clamp with two static bounds, lo <= hi --
    as conv2d_qc's act_min / act_max (None: no bound on that side); None for any other node."""
    a = torch.ops.aten
    if getattr(node, "op", None) != "call_function":
        return None
    if node.target in (a.relu.default, a.relu_.default):
        return (0.0, None) if len(node.args) == 1 and not node.kwargs else None
    if node.target in (a.hardtanh.default, a.hardtanh_.default):
        names, vals = ("min_val", "max_val"), [-1.0, 1.0]
    elif node.target == a.clamp.default:
        names, vals = ("min", "max"), [None, None]
    else:
        return None
    if not 1 <= len(node.args) <= 3 or any(k not in names for k in node.kwargs):
        return None
    vals[:len(node.args) - 1] = node.args[1:]
    for i, k in enumerate(names):
        vals[i] = node.kwargs.get(k, vals[i])
    if not all(_static_number(v) for v in vals) or any(v != v for v in vals) or not vals[0] <= vals[1]:
        return None
    return float(vals[0]), float(vals[1])


def _attr_of(model, node):
    """The tensor behind a get_attr node, else None."""
    if getattr(node, "op", None) != "get_attr":
        return None
    obj = model
    for part in str(node.target).split("."):
        obj = getattr(obj, part, None)
    return obj if isinstance(obj, torch.Tensor) else None


def _conv_q_node(node):
    """"q" for a conv2d_q node, "qc" for a conv2d_qc node, else None."""
    ops = torch.ops.quantized_ops
    if _is(node, ops.conv2d_q.default) and len(node.args) == 12 and not node.kwargs:
        return "q"
    if _is(node, ops.conv2d_qc.default) and len(node.args) == 16 and not node.kwargs:
        return "qc"
    return None


def _node_shape(model, node, seen):
    """(shape, dtype) of a graph node's value tensor: meta["val"] where the node has one; a conv2d_q / conv2d_qc node (fusion leaves
    them without one) from its input's shape, its weight codes and _conv_out_hw, in out_scale's dtype; an activation from its input.
    None when nothing static says."""
    if not isinstance(node, torch.fx.Node) or node in seen:
        return None
    val = node.meta.get("val")
    if isinstance(val, torch.Tensor) and all(isinstance(d, int) for d in val.shape):
        return tuple(val.shape), val.dtype
    seen = seen | {node}
    if _conv_q_node(node):
        src, w, s = _node_shape(model, node.args[0], seen), _attr_of(model, node.args[3]), _attr_of(model, node.args[9])
        if src is None or w is None or s is None or len(src[0]) != 4 or w.dim() != 4:
            return None
        ho, wo = _conv_out_hw(src[0][2], src[0][3], w.shape[1], w.shape[2], *node.args[5:8])
        return (src[0][0], w.shape[0], ho, wo), s.dtype
    if _chain_activation(node) is not None:
        return _node_shape(model, node.args[0], seen)
    return None


def _chain_declines(model, node, in_shape):
    """_conv_q_decline for a conv2d_q / conv2d_qc node whose input has the static shape `in_shape`, as for a device call (the rule part
    under _APPLY_CONV_Q_RULE, as everywhere).  An operand that is not a buffer of the model declines: nothing static says what it is."""
    w, s_out = _attr_of(model, node.args[3]), _attr_of(model, node.args[9])
    bias = _attr_of(model, node.args[4]) if node.args[4] is not None else None
    if w is None or s_out is None or (node.args[4] is not None and bias is None):
        return "an operand that is not a buffer"
    dtype = s_out.dtype
    if node.args[1] is None:                             # already takes codes
        scale, qmap = _Operand((1,), dtype, w.device), _Operand((65536,), torch.bfloat16, w.device)
    else:
        scale, qmap = _attr_of(model, node.args[1]), _attr_of(model, node.args[2])
        if scale is None or qmap is None:
            return "an operand that is not a buffer"
    return _conv_q_decline(_Operand(in_shape, dtype, w.device), scale, qmap, w, bias, *node.args[5:9], s_out, node.args[11], on_device=True)


def fuse_conv_q_chains(model: GraphModule) -> int:
    """Hands int8 codes from one converted convolution to the next.  For a producer P (a conv2d_q node, or a conv2d_qc node that still
    writes values) whose sole user is an activation T of _chain_activation -- or T = P -- and whose T feeds nothing but conv2d_q nodes,
    each as its `input` alone, all quantizing with the same scale node and the same map node:
        P            -> conv2d_qc(..., act_min, act_max, that scale, that map)      codes out (qt_q8_*_codes)
        T            erased
        each user    -> conv2d_qc(P, None, None, ...)                                codes in: no codes pass
    A consumer that is a producer in turn becomes one node that does both.  An edge is rewritten only where the kernels take both
    ends as a device call would (P's Cout a multiple of 16, _conv_q_decline None for P and every consumer on the static shapes of
    the graph): anywhere else it would only add fallback passes.  A tail with any other user (a residual add, the graph output, a
    pooling), any other activation, a bound that is a tensor, unknown shapes: left exactly as they are.  Idempotent; run after
    fuse_native_gemms.  Returns the number of producer -> consumer edges rewritten."""
    ops = torch.ops.quantized_ops
    graph = model.graph
    edges = 0
    for p in list(graph.nodes):
        kind = _conv_q_node(p)
        if kind is None or (kind == "qc" and p.args[14] is not None):
            continue
        tail, bounds = p, (None, None)
        users = list(p.users)
        if len(users) == 1 and _conv_q_node(users[0]) is None:
            bounds = _chain_activation(users[0])
            if bounds is None or users[0].args[0] is not p:
                continue
            tail = users[0]
        consumers = list(tail.users)
        if not consumers or any(_conv_q_node(c) is None or c.args[0] is not tail or c.args[1] is None
                                or any(a is tail for a in c.args[1:]) for c in consumers):
            continue
        s_node, m_node = consumers[0].args[1], consumers[0].args[2]
        if any(c.args[1] is not s_node or c.args[2] is not m_node for c in consumers) or s_node.op != "get_attr" or m_node.op != "get_attr":
            continue
        w = _attr_of(model, p.args[3])
        src, mid = _node_shape(model, p.args[0], frozenset()), _node_shape(model, p, frozenset())
        if w is None or w.shape[0] % 16 or src is None or mid is None or len(src[0]) != 4:
            continue
        if _chain_declines(model, p, src[0]) is not None or any(_chain_declines(model, c, mid[0]) is not None for c in consumers):
            continue
        for n in (s_node, m_node):                       # the consumer's scale and map now feed the producer
            if n in p.all_input_nodes:
                continue
            for earlier in graph.nodes:
                if earlier is p:
                    p.prepend(n)
                    break
                if earlier is n:
                    break
        p.target = ops.conv2d_qc.default
        p.args = (*p.args[:12], bounds[0], bounds[1], s_node, m_node)
        p.meta.pop("val", None)
        if tail is not p:
            tail.replace_all_uses_with(p)
            graph.erase_node(tail)
        for c in consumers:
            c.target = ops.conv2d_qc.default
            c.args = (p, None, None, *c.args[3:12], *(c.args[12:] if len(c.args) == 16 else (None, None, None, None)))
            edges += 1
    if edges:
        graph.eliminate_dead_code(is_impure_node=lambda n: n.op in {"placeholder", "output"})
        graph.lint()
        model.recompile()
    return edges


def _is_mx_consumer(node):
    ops = torch.ops.quantized_ops
    return getattr(node, "op", None) == "call_function" and node.target in (ops.linear_mx.default, ops.matmul_mx.default,
                                                                            ops.conv2d_mx.default)


def _axes_list(axes):
    """The `axes` argument of a graph node as a list of ints (a hand-built graph may carry a bare int), else None."""
    if isinstance(axes, int) and not isinstance(axes, bool):
        return [axes]
    if isinstance(axes, (list, tuple)) and all(isinstance(a, int) and not isinstance(a, bool) for a in axes):
        return list(axes)
    return None


def fuse_mx_pairs(model: GraphModule) -> int:
    """Folds `s = calculate_mx_qparam(x, axes, bs, qmax, pow2[, smap])` + `quantize(x, s, None, axes, bs, qmap, None)` -- what
    convert_pt2e emits for an activation whose blocks do not run along the last axis (the second operand of every block-scaled
    matmul, quantize_pt2e.py: `_with_axis(activation, -2)`) -- into one `quantize_mx(x, qmap, axes, bs, qmax, pow2, smap, None)`
    node with two getitems, so that the device runs one pass over x (and gets the packed matmul operand with it).  quantize_mx's
    fallback is literally those two ops, so the fold changes no result on any device or dtype.  Returns the number of folds."""
    import operator
    ops = torch.ops.quantized_ops
    graph = model.graph
    order = {n: i for i, n in enumerate(graph.nodes)}
    fused = 0
    for q in list(graph.nodes):
        if not _is(q, ops.quantize.default) or q.kwargs or len(q.args) < 6:
            continue
        a = list(q.args) + [None] * (7 - len(q.args))
        src, s, zp, axes, bs, qmap, code = a[:7]
        if not _is(s, ops.calculate_mx_qparam.default) or s.kwargs or zp is not None or code is not None or qmap is None:
            continue
        if not 4 <= len(s.args) <= 6:
            continue
        sa = list(s.args) + [False, None][len(s.args) - 4:]        # (x, axes, bs, qmax, pow2, smap)
        if sa[0] is not src or getattr(src, "op", "get_attr") == "get_attr":
            continue
        s_axes, q_axes = _axes_list(sa[1]), _axes_list(axes)
        if s_axes is None or s_axes != q_axes or sa[2] != bs:      # axes that are no int or sequence of ints: leave the pair
            continue
        if any(u is not q and (not _is_mx_consumer(u) or order[u] < order[q]) for u in s.users):
            continue
        with graph.inserting_before(q):                             # behind the map's get_attr; every user of s comes after q
            mx = graph.call_function(ops.quantize_mx.default, (src, qmap, s_axes if isinstance(sa[1], int) else sa[1], bs, sa[3], sa[4], sa[5], None))
            s_new = graph.call_function(operator.getitem, (mx, 0))
            q_new = graph.call_function(operator.getitem, (mx, 1))
        # the fused branch of quantize_pt2e._lower_mx_fake_quant: (scale dtype, element dtype) on the node, each on its getitem
        mx.meta["dtype"] = (s.meta.get("dtype"), q.meta.get("dtype"))
        if "source_fn_stack" in q.meta:
            mx.meta["source_fn_stack"] = [(mx.name, mx.target)]
        s_new.meta, q_new.meta = dict(s.meta), dict(q.meta)
        q_new.meta.pop("source_fn_stack", None)
        q.replace_all_uses_with(q_new)
        s.replace_all_uses_with(s_new)
        graph.erase_node(q)
        graph.erase_node(s)
        fused += 1
    if fused:
        graph.lint()
        model.recompile()
    return fused


def enabled_for(model) -> bool:
    if not switches.on("QT_PT2E_NATIVE"):
        return False
    try:
        return next(iter(model.parameters())).device.type == "cuda"
    except StopIteration:
        return False


# ---- packed group-wise affine weights: dequantize + aten.linear -> linear_gwa (csrc/qt_gwa_gemm.hip) ----------------------------------
# convert_pt2e leaves, for a `uintN,qs=group_wise_affine,bs=..,ax=-1` Linear weight, three bf16 buffers (codes, scales, zero points)
# and `dequantize(codes, scale, zero_point, (-1,), bs)` in front of aten.linear.  fuse_gwa_linears stores the codes packed (4 or 8
# bits each instead of 16) and rewrites the pair into one linear_gwa node; on the device that node runs the fused
# dequantize-GEMM where the committed rule takes the shape and the one-pass dequantize kernel + the library GEMM elsewhere.
GWA_BLOCKS = (32, 64, 128, 256, 512)
GWA_TILES = (16, 32, 64)                  # row-tile heights of qt_linear_gwa_bf16 (tile_m; 0 = by M)
GWA_ROUTES = {}                           # "gwa:MxNxK" -> route of the first call with that shape (fused.routes_report)


class _GwaStats:
    """Calls of linear_gwa per route, and why a device call did not take the fused kernel."""
    def __init__(self):
        self.reset()

    def reset(self):
        self.fused = self.dequant = self.reference = 0
        self.reasons = {}

    def note(self, why):
        self.reasons[why] = self.reasons.get(why, 0) + 1


GWA_STATS = _GwaStats()

_lib.define("linear_gwa(Tensor input, Tensor packed, Tensor scale, Tensor zero_point, Tensor? bias, int block_size, int quant_min, "
            "int bits, int K) -> Tensor")


def gwa_dtype_range(dtype):
    """(quant_min, quant_max, bits) of an integer element dtype of at most 8 bits ("uint4", "int4", "uint2", "uint8", ...), else None."""
    import re
    m = re.fullmatch(r"(u?)int(\d+)", str(dtype).split(",")[0].strip())
    if m is None or not 1 <= int(m.group(2)) <= 8:
        return None
    n = int(m.group(2))
    lo, hi = (0, 2 ** n - 1) if m.group(1) else (-(2 ** (n - 1)), 2 ** (n - 1) - 1)
    return lo, hi, 4 if hi - lo <= 15 else 8


def _gwa_geometry(N, K, bits):
    j = 4 if bits == 4 else 2              # k steps of 32 per super step
    return (N + 15) // 16, (K + 32 * j - 1) // (32 * j), j


def gwa_pack_torch(codes, quant_min, quant_max, bits):
    """The packed layout of qt_gwa_pack in torch ops (include/qt_hip.h): uint8 [bytes], or None when a code is not an integer in
    [quant_min, quant_max]."""
    N, K = codes.shape
    c = codes.detach().to(torch.float32)
    if not bool(((c == c.round()) & (c >= quant_min) & (c <= quant_max)).all()):
        return None
    n16, nss, j = _gwa_geometry(N, K, bits)
    q = torch.zeros((n16 * 16, nss * 32 * j), dtype=torch.uint8, device=codes.device)
    q[:N, :K] = (c - quant_min).to(torch.uint8)
    q = q.view(n16, 16, nss, j, 4, 8).permute(0, 2, 4, 1, 3, 5)           # [group, super step, g, r, k step, e]
    if bits == 4:
        q = q[..., 0::2] | (q[..., 1::2] << 4)
    return q.contiguous().view(-1)


def gwa_unpack_torch(packed, N, K, bits):
    """Inverse of the packers: uint8 codes - quant_min, [N, K]."""
    n16, nss, j = _gwa_geometry(N, K, bits)
    p = packed.view(n16, nss, 4, 16, j, 4 if bits == 4 else 8)
    if bits == 4:
        p = torch.stack((p & 15, p >> 4), dim=-1).view(n16, nss, 4, 16, j, 8)
    return p.permute(0, 3, 1, 4, 2, 5).reshape(n16 * 16, nss * 32 * j)[:N, :K]


def _gwa_shape_ok(N, K, block_size):
    return (isinstance(block_size, int) and not isinstance(block_size, bool) and block_size in GWA_BLOCKS and K % block_size == 0
            and K % 32 == 0 and N % 8 == 0 and N > 0)


def gwa_pack(codes, quant_min, quant_max, bits):
    """Packed operand of a [N, K] codes tensor, or None when the check fails (or the shape is not the kernels').  Device bf16 codes go
    through qt_gwa_pack and its flag -- read by the host here, once, at convert time -- everything else through the torch ops."""
    N, K = codes.shape
    if codes.device.type == "cuda" and codes.dtype == torch.bfloat16 and K % 32 == 0 and N % 8 == 0:
        L = _native.lib()
        c = codes.detach().contiguous()
        nbytes = L.qt_gwa_packed_bytes(N, K, bits)
        if nbytes:
            packed = torch.empty(nbytes, dtype=torch.uint8, device=c.device)
            bad = torch.zeros(1, dtype=torch.int32, device=c.device)
            rc = L.qt_gwa_pack(c.data_ptr(), packed.data_ptr(), N, K, bits, float(quant_min), float(quant_max), bad.data_ptr(),
                               _stream_ptr(c))
            if not _native.declined(rc):
                _native.check(rc, "qt_gwa_pack")
                return None if int(bad.item()) != 0 else packed
    return gwa_pack_torch(codes, quant_min, quant_max, bits)


def _gwa_reference(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K):
    """The unfused graph on the unpacked codes: bit for bit what dequantize + aten.linear computed."""
    codes = gwa_unpack_torch(packed, scale.shape[0], K, bits).to(scale.dtype) + quant_min
    w = torch.ops.quantized_ops.dequantize(codes, scale, zero_point, (-1,), block_size)
    return torch.nn.functional.linear(input, w, bias)


_GWA_FUSED_MAX_M = 32


def _gwa_route_takes(M, N, K):
    """The committed rule, a fixed function of the problem (never a timing).  From profiles/gwa_linear.txt (uint4, bs = 128, LLaMA-2-7B's
    three projection shapes, weights rotating beyond the Infinity Cache): at M = 1, 16 and 32 the fused kernel's slowest round beats the
    fastest round of qt_gwa_dequantize_bf16 + the library GEMM on every weight (1.6 - 2.8 x at the medians); at M = 64 it does so on
    two weights of three (it ties on 11008 x 4096), at M = 128 on one, at M = 1024 on none (0.2 x: every 64-row tile converts the
    weight again).  A shape class goes to the fused kernel only where it won every row: M <= 32."""
    return M <= _GWA_FUSED_MAX_M


def gwa_dequantize(packed, scale, zero_point, block_size, quant_min, bits, K):
    """qt_gwa_dequantize_bf16: the bf16 weight [N, K] in one pass, or None when the kernel declines."""
    N = scale.shape[0]
    w = torch.empty((N, K), dtype=torch.bfloat16, device=packed.device)
    rc = _native.lib().qt_gwa_dequantize_bf16(packed.data_ptr(), scale.data_ptr(), zero_point.data_ptr(), w.data_ptr(), N, K,
                                              block_size, bits, float(quant_min), _stream_ptr(packed))
    if _native.declined(rc):
        return None
    _native.check(rc, "qt_gwa_dequantize_bf16")
    return w


def linear_gwa_route(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K, route=None, tile_m=0):
    """linear_gwa with the route in the caller's hands: None = the committed rule, "fused" / "dequant" / "reference" = that route
    (a forced route the kernels decline falls through to the next one, as the rule's does), tile_m = the fused kernel's variant."""
    N = scale.shape[0]
    device_ok = (input.device.type == "cuda" and input.dtype == torch.bfloat16 and scale.dtype == torch.bfloat16
                 and zero_point.dtype == torch.bfloat16 and packed.dtype == torch.uint8 and input.shape[-1] == K
                 and _gwa_shape_ok(N, K, block_size) and bits in (4, 8) and input.numel() > 0
                 and (bias is None or bias.dtype == torch.bfloat16))
    M = input.numel() // K if K else 0
    key = f"gwa:{M}x{N}x{K}"
    if route == "reference" or not device_ok:
        if route != "reference":
            GWA_STATS.note("not a bf16 device call the kernels take")
        GWA_STATS.reference += 1
        GWA_ROUTES.setdefault(key, "unpack+dequantize+linear")
        return _gwa_reference(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K)
    L = _native.lib()
    s, z = scale.contiguous(), zero_point.contiguous()
    if route == "fused" or (route is None and _gwa_route_takes(M, N, K)):
        x = input.reshape(M, K).contiguous()
        b = bias.contiguous() if bias is not None else None
        y = torch.empty((M, N), dtype=torch.bfloat16, device=input.device)
        rc = L.qt_linear_gwa_bf16(x.data_ptr(), packed.data_ptr(), s.data_ptr(), z.data_ptr(), b.data_ptr() if b is not None else None,
                                  y.data_ptr(), M, N, K, block_size, bits, float(quant_min), tile_m, _stream_ptr(x))
        if not _native.declined(rc):
            _native.check(rc, "qt_linear_gwa_bf16")
            GWA_STATS.fused += 1
            GWA_ROUTES.setdefault(key, "fused_gwa_gemm")
            return y.view(*input.shape[:-1], N)
        GWA_STATS.note("qt_linear_gwa_bf16 declined")
    elif route is None:
        GWA_STATS.note("route rule")
    w = gwa_dequantize(packed, s, z, block_size, quant_min, bits, K)
    if w is None:
        GWA_STATS.note("qt_gwa_dequantize_bf16 declined")
        GWA_STATS.reference += 1
        GWA_ROUTES.setdefault(key, "unpack+dequantize+linear")
        return _gwa_reference(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K)
    GWA_STATS.dequant += 1
    GWA_ROUTES.setdefault(key, "gwa_dequantize+library_gemm")
    return torch.nn.functional.linear(input, w, bias)


def _linear_gwa(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K):
    return linear_gwa_route(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K)


def _linear_gwa_meta(input, packed, scale, zero_point, bias, block_size, quant_min, bits, K):
    return input.new_empty((*input.shape[:-1], scale.shape[0]))


_lib.impl("linear_gwa", _linear_gwa, "CompositeExplicitAutograd")
_lib.impl("linear_gwa", _linear_gwa_meta, "Meta")


def _owner_and_name(model, target):
    mod, _, name = str(target).rpartition(".")
    return (model.get_submodule(mod) if mod else model), name


def fuse_gwa_linears(model: GraphModule) -> int:
    """Rewrites `dequantize(codes, scale, zero_point, (last axis,), bs)` + `aten.linear` of a bf16 model into one `linear_gwa` node on
    the packed codes (buffer `<codes>_packed`; the bf16 codes buffer is deleted when nothing else reads it).  Fused only when the
    three operands are bf16 get_attr buffers, there are no maps, the blocks run along the weight's last axis with an int block
    size the kernels take, the dequantize's sole user is an aten.linear that uses it as the weight, and every code passes the
    packer's check; everything else keeps its two nodes.  Returns the number of fused Linears."""
    DQ = torch.ops.quantized_ops.dequantize.default
    graph = model.graph
    fused = 0
    for dq in list(graph.nodes):
        if not _is(dq, DQ) or dq.kwargs or not 5 <= len(dq.args) <= 7:
            continue
        a = list(dq.args) + [None] * (7 - len(dq.args))
        q, s, z, axes, bs = a[:5]
        if a[5] is not None or a[6] is not None or z is None:
            continue
        if any(getattr(n, "op", None) != "get_attr" for n in (q, s, z)):
            continue
        users = list(dq.users.keys())
        if len(users) != 1 or not _is(users[0], torch.ops.aten.linear.default):
            continue
        lin = users[0]
        if lin.kwargs or len(lin.args) < 2 or lin.args[1] is not dq or lin.args[0] is dq or (len(lin.args) > 2 and lin.args[2] is dq):
            continue
        try:
            codes, scale, zero = (model.get_buffer(n.target) for n in (q, s, z))
        except AttributeError:
            continue
        if any(t.dtype != torch.bfloat16 for t in (codes, scale, zero)) or codes.dim() != 2:
            continue
        ax = _axes_list(axes)
        if ax is None or len(ax) != 1 or ax[0] % codes.dim() != codes.dim() - 1:
            continue
        N, K = codes.shape
        if not _gwa_shape_ok(N, K, bs) or tuple(scale.shape) != (N, K // bs) or tuple(zero.shape) != (N, K // bs):
            continue
        rng = gwa_dtype_range(q.meta.get("dtype"))
        if rng is None:
            continue
        qmin, qmax, bits = rng
        packed = gwa_pack(codes, qmin, qmax, bits)
        if packed is None:
            continue                                         # a code the packed form cannot hold: keep the value tensor
        owner, leaf = _owner_and_name(model, q.target)
        name, i = leaf + "_packed", 0
        while hasattr(owner, name):
            i += 1
            name = f"{leaf}_packed_{i}"
        owner.register_buffer(name, packed)
        prefix = str(q.target).rpartition(".")[0]
        bias = lin.args[2] if len(lin.args) > 2 else None
        with graph.inserting_before(lin):
            p_node = graph.create_node("get_attr", (prefix + "." if prefix else "") + name)
            new = graph.call_function(torch.ops.quantized_ops.linear_gwa.default,
                                      (lin.args[0], p_node, s, z, bias, bs, int(qmin), bits, K))
        p_node.meta["dtype"] = q.meta.get("dtype")
        new.meta = dict(lin.meta)
        lin.replace_all_uses_with(new)
        graph.erase_node(lin)
        graph.erase_node(dq)
        if len(q.users) == 0:
            graph.erase_node(q)
            if not any(n.op == "get_attr" and n.target == q.target for n in graph.nodes):
                delattr(owner, leaf)                         # 2 bytes per weight -> 0.5 (or 1)
        fused += 1
    if fused:
        graph.lint()
        model.recompile()
    return fused
