"""attention_mx on the block-scaled attention cores: integer operands (csrc/qt_attention_mxi.hip) and, in front of them, the float
formats of the scaled matrix instruction (csrc/qt_attention_mxf.hip; the section "The float core" below).

A converted graph of the block-scaled integer recipe holds, per attention layer,
    matmul_mx(q, k^T) -> mul / div by a scalar -> + mask -> softmax(-1) -> quantize_mx(p, ax=-1) -> matmul_mx(p', v)
between the `quantize_mx` nodes of q, k^T and v.  pt2e_native.fuse_mx_attention folds that span into one
`quantized_ops::attention_mx` node (decomposed.py); this module is the node's device route: the three operands are packed with
qt_mxi_pack exactly as mx_gemm._int_matmul packs them (trusting the integer record or the codebook that mx_operand keeps) and
qt_attention_mxi runs the span with every rounding of the nodes kept.  What the kernel's contract or the route rule does not take
returns None, is counted, and the operator runs the replaced nodes literally.

Contract: bf16, block size 64 for all four operands, head_dim 64 or 128, a key count that is a multiple of 64 in 64 .. 16384,
B H <= 65535, P quantized to an `intN` map (N <= 8) with amax / qmax scales (optionally through a scale map) or power-of-two scales,
a bf16 mask that broadcasts to [B, H, Q, C] with contiguous keys, 8-byte aligned, strides that are multiples of 4.
"""
import ctypes

import torch

from . import _native, mx_gemm, mx_operand, switches
from .fake_quantize import _stream_ptr

__all__ = ["attention_mx_or_none", "pack_operands", "launch", "pack_operands_mxf", "launch_mxf", "STATS", "ATTENTION_MXI_ROUTES"]

STATS = {"attention_native": 0, "attention_fallback": 0}        # calls of the operator on device tensors, by route
ATTENTION_MXI_ROUTES = {}                 # "attention_mxi:BxHxQxCxD" | "attention_mxf:BxHxQxCxD" -> route of the first call with that shape (fused.routes_report)
_DEBUG = False                            # set mx_attention._DEBUG = True to print why a call ran the nodes

# (B, H, Q, C, D) -> does the packs + qt_attention_mxi route beat the span of nodes?  The bar of attention_route._FP8_LONG_TABLE: a class
# is listed when the kernel route's median beats the nodes' by more than the nodes' min-max spread, eager AND replayed from a graph, with
# the causal mask AND without a mask (tools/exp_attention_mxi.py -> profiles/attention_mxi.txt).  The table lists exactly the classes
# that cleared it.
_MXI_ATTENTION_TABLE = {
    (1, 32, 512, 512, 128): True, (1, 32, 1024, 1024, 128): True, (1, 32, 2048, 2048, 128): True, (1, 32, 4096, 4096, 128): True,
    (4, 12, 512, 512, 64): True, (4, 12, 2048, 2048, 64): True,
}


def _mxi_attention_route_takes(B, H, Q, C, D):
    """The default route: the committed table, a fixed function of the shape; a shape it does not list stays on the nodes.  Never a
    measurement at run time (fused.fq8_route_is_fused says why)."""
    return _MXI_ATTENTION_TABLE.get((B, H, Q, C, D), False)


def _decline(why, key=None):
    STATS["attention_fallback"] += 1
    if key is not None:
        ATTENTION_MXI_ROUTES.setdefault(key, "nodes")
    if _DEBUG:
        print("mx_attention: the nodes:", why, flush=True)
    return None


def _table_ok(m):
    return m.dtype == torch.bfloat16 and m.numel() == 65536 and m.is_contiguous()


def _mask_strides(mask, B, H, Q, C):
    """(b, h, q) element strides of a mask the kernel reads in place, or None."""
    if mask.dtype != torch.bfloat16 or mask.dim() > 4 or mask.dim() < 1 or mask.shape[-1] != C or mask.stride(-1) != 1:
        return None
    try:
        sb, sh, sq, _ = mask.expand(B, H, Q, C).stride()
    except RuntimeError:
        return None
    if mask.data_ptr() % 8 or sb % 4 or sh % 4 or sq % 4:
        return None
    return sb, sh, sq


def attention_mx_or_none(q, q_scale, kT, kT_scale, v, v_scale, mask, scaling, scaling_is_div, p_qmap, p_quant_max, p_pow2, p_scale_qmap,
                         block_size, q_code, k_code, v_code):
    """The result [B, H, Q, D] on the kernel route, or None (counted) for a call the operator runs as the replaced nodes."""
    if q.device.type != "cuda":
        return None
    if not switches.on("QT_MX_GEMM") or switches.mode("QT_FUSED_ATTENTION") == "0":
        return _decline("switched off")
    fid = _mxf_format(q, q_scale, kT, kT_scale, v, v_scale, p_qmap, p_pow2, p_scale_qmap, block_size)
    if fid is not None:
        return _attention_mxf(fid, q, q_scale, kT, kT_scale, v, v_scale, mask, scaling, scaling_is_div, p_qmap, p_quant_max)
    if block_size != 64 or isinstance(block_size, bool):
        return _decline(f"block size {block_size}")
    ts = (q, q_scale, kT, kT_scale, v, v_scale)
    if any(t.dtype != torch.bfloat16 or t.device != q.device for t in ts) or q.dim() != 4 or kT.dim() != 4 or v.dim() != 4:
        return _decline("not bf16 [B, H, ., .] operands on one device")
    B, H, Q, D = q.shape
    C = kT.shape[3]
    nd, nc = D // 64, C // 64
    if D not in (64, 128) or C % 64 or not 64 <= C <= 16384 or Q < 1 or B * H < 1 or B * H > 65535:
        return _decline(f"shape B {B} H {H} Q {Q} C {C} D {D}")
    if tuple(kT.shape) != (B, H, D, C) or tuple(v.shape) != (B, H, C, D) or tuple(q_scale.shape) != (B, H, Q, nd) \
            or tuple(kT_scale.shape) != (B, H, nd, C) or tuple(v_scale.shape) != (B, H, nc, D):
        return _decline("operand or scale shapes")
    key = f"attention_mxi:{B}x{H}x{Q}x{C}x{D}"
    if not all(mx_gemm._int_operand_ok(t, c) for t, c in ((q, q_code), (kT, k_code), (v, v_code))):
        return _decline("an operand without an integer record or codebook", key)
    p_name = mx_operand.int_format_of_qmap(p_qmap)
    if p_name is None or p_qmap.device != q.device:
        return _decline("P's map is not a tagged intN map", key)
    if not p_quant_max > 0 or (p_scale_qmap is not None and (p_pow2 or not _table_ok(p_scale_qmap) or p_scale_qmap.device != q.device)):
        return _decline("P's scale arguments", key)
    strides = (0, 0, 0)
    if mask is not None:
        strides = _mask_strides(mask, B, H, Q, C) if mask.device == q.device else None
        if strides is None:
            return _decline("a mask the kernel does not read in place", key)
    if switches.mode("QT_FUSED_ATTENTION") != "1" and not _mxi_attention_route_takes(B, H, Q, C, D):
        return _decline("the route rule keeps the nodes", key)
    packed = pack_operands(q, q_scale, kT, kT_scale, v, v_scale, q_code, k_code, v_code)
    out = torch.empty((B, H, Q, D), dtype=torch.bfloat16, device=q.device)
    code = launch(packed, mask, strides, scaling, scaling_is_div, p_name, p_quant_max, p_pow2, p_scale_qmap, out)
    if _native.declined(code):
        return _decline(f"qt_attention_mxi declined ({code})", key)
    _native.check(code, "qt_attention_mxi")
    STATS["attention_native"] += 1
    ATTENTION_MXI_ROUTES.setdefault(key, "qt_attention_mxi")
    return out


def pack_operands(q, q_scale, kT, kT_scale, v, v_scale, q_code=None, k_code=None, v_code=None):
    """The three packs of mx_gemm._int_matmul, check off: q [B, H, Q, D] as a first operand; k^T [B, H, D, C] and v [B, H, C, D] as second
    operands (logical rows are their columns).  -> ((codes, scales) of q, of k, of v)."""
    B, H, Q, D = q.shape
    C = kT.shape[3]
    BH, nd, nc = B * H, D // 64, C // 64
    pq = mx_gemm._int_pack(q.contiguous(), q_scale.contiguous(), q_code, 64, BH, Q, D, (Q * D, D, 1), (Q * nd, nd, 1), check=False)
    k3, xk = mx_gemm._rows_view(kT, BH, C, D)
    sk3, xsk = mx_gemm._rows_view(kT_scale, BH, C, nd)
    pk = mx_gemm._int_pack(k3, sk3, k_code, 64, BH, C, D, xk, xsk, check=False)
    v3, xv = mx_gemm._rows_view(v, BH, D, C)
    sv3, xsv = mx_gemm._rows_view(v_scale, BH, D, nc)
    pv = mx_gemm._int_pack(v3, sv3, v_code, 64, BH, D, C, xv, xsv, check=False)
    return pq, pk, pv


def launch(packed, mask, mask_strides, scaling, scaling_is_div, p_name, p_quant_max, p_pow2, p_scale_qmap, out, block_size=64):
    """qt_attention_mxi on packed operands into `out` [B, H, Q, D] bf16 (its scratch is allocated here).  Returns the status code."""
    pq, pk, pv = packed
    B, H, Q, D = out.shape
    BH, C = pq[0].shape[0], pk[0].shape[1]
    v_work = torch.empty_like(pv[0])
    vs_work = torch.empty((BH, max(C // 64, 1), D), dtype=torch.float32, device=out.device)
    fmt = _native.format_for(p_name)
    return _native.lib().qt_attention_mxi(
        pq[0].data_ptr(), pq[1].data_ptr(), pk[0].data_ptr(), pk[1].data_ptr(), pv[0].data_ptr(), pv[1].data_ptr(), v_work.data_ptr(),
        vs_work.data_ptr(), mask.data_ptr() if mask is not None else None, *mask_strides, float(scaling), int(bool(scaling_is_div)),
        ctypes.byref(fmt), float(p_quant_max), int(bool(p_pow2)), p_scale_qmap.data_ptr() if p_scale_qmap is not None else None,
        out.data_ptr(), B, H, Q, C, D, block_size, _stream_ptr(out))


# ---- The float core: fp8_e4m3 / fp8_e5m2 / fp4_e2m1 under block size 32 and power-of-two scales (csrc/qt_attention_mxf.hip) ----------
# Contract: bf16, block size 32 for all four operands, ONE element format for q, k^T, v and P, power-of-two scales (P's forced, no
# scale map), head_dim 64 or 128, a key count that is a multiple of 128 in 128 .. 16384, B H <= 65535, the mask as above.  The kernel
# reads the packed operands quantize_mx already wrote (mx_operand's records); an operand without one is packed here, check off.

# (B, H, Q, C, D) -> does qt_attention_mxf beat the span of nodes?  The bar of _MXI_ATTENTION_TABLE, for fp8_e4m3 AND fp4_e2m1
# (tools/exp_attention_mxf.py -> profiles/attention_mxf.txt).  The table lists exactly the classes that cleared it.
_MXF_ATTENTION_TABLE = {
    (1, 32, 512, 512, 128): True, (1, 32, 1024, 1024, 128): True, (1, 32, 2048, 2048, 128): True, (1, 32, 4096, 4096, 128): True,
    (4, 12, 512, 512, 64): True, (4, 12, 2048, 2048, 64): True,
}


def _mxf_attention_route_takes(B, H, Q, C, D):
    """The default route of the float core: the committed table, a fixed function of the shape."""
    return _MXF_ATTENTION_TABLE.get((B, H, Q, C, D), False)


def _mxf_format(q, q_scale, kT, kT_scale, v, v_scale, p_qmap, p_pow2, p_scale_qmap, block_size):
    """The QT_MX_* id when the call is the float core's to answer -- block size 32, forced power-of-two scales for P without a scale
    map, one of the three formats on q, k^T, v and P's map alike, power-of-two scales on all three operands -- else None."""
    if block_size != 32 or isinstance(block_size, bool) or not p_pow2 or p_scale_qmap is not None:
        return None
    name = mx_operand.format_of(q)
    if name not in ("fp8_e4m3", "fp8_e5m2", "fp4_e2m1") or mx_operand.format_of(kT) != name or mx_operand.format_of(v) != name \
            or mx_operand.format_of_qmap(p_qmap) != name:
        return None
    if not all(mx_operand.is_pow2(s) for s in (q_scale, kT_scale, v_scale)):
        return None
    return mx_operand.FMT_ID[name]


def _attention_mxf(fid, q, q_scale, kT, kT_scale, v, v_scale, mask, scaling, scaling_is_div, p_qmap, p_quant_max):
    ts = (q, q_scale, kT, kT_scale, v, v_scale, p_qmap)
    if any(t.dtype != torch.bfloat16 or t.device != q.device for t in ts) or q.dim() != 4 or kT.dim() != 4 or v.dim() != 4:
        return _decline("not bf16 [B, H, ., .] operands on one device")
    B, H, Q, D = q.shape
    C = kT.shape[3]
    nd, nc = D // 32, C // 32
    if D not in (64, 128) or C % 128 or not 128 <= C <= 16384 or Q < 1 or B * H < 1 or B * H > 65535:
        return _decline(f"shape B {B} H {H} Q {Q} C {C} D {D}")
    if tuple(kT.shape) != (B, H, D, C) or tuple(v.shape) != (B, H, C, D) or tuple(q_scale.shape) != (B, H, Q, nd) \
            or tuple(kT_scale.shape) != (B, H, nd, C) or tuple(v_scale.shape) != (B, H, nc, D):
        return _decline("operand or scale shapes")
    key = f"attention_mxf:{B}x{H}x{Q}x{C}x{D}"
    if not p_quant_max > 0 or p_qmap.numel() != 65536 or not p_qmap.is_contiguous():
        return _decline("P's quantizer arguments", key)
    strides = (0, 0, 0)
    if mask is not None:
        strides = _mask_strides(mask, B, H, Q, C) if mask.device == q.device else None
        if strides is None:
            return _decline("a mask the kernel does not read in place", key)
    if switches.mode("QT_FUSED_ATTENTION") != "1" and not _mxf_attention_route_takes(B, H, Q, C, D):
        return _decline("the route rule keeps the nodes", key)
    packed = pack_operands_mxf(fid, q, q_scale, kT, kT_scale, v, v_scale)
    out = torch.empty((B, H, Q, D), dtype=torch.bfloat16, device=q.device)
    code = launch_mxf(fid, packed, mask, strides, scaling, scaling_is_div, p_qmap, p_quant_max, out)
    if _native.declined(code):
        return _decline(f"qt_attention_mxf declined ({code})", key)
    _native.check(code, "qt_attention_mxf")
    STATS["attention_native"] += 1
    ATTENTION_MXI_ROUTES.setdefault(key, "qt_attention_mxf")
    return out


def pack_operands_mxf(fid, q, q_scale, kT, kT_scale, v, v_scale):
    """The packed operands as mx_gemm._float_matmul finds them: the record quantize_mx left (q under ROWS; k^T and v under SECOND, their
    logical rows being their columns), or a pack with the check off.  -> ((codes, e8m0) of q, of k, of v)."""
    B, H, Q, D = q.shape
    C = kT.shape[3]
    BH = B * H

    def second(t, s, rows, k):                   # t [B, H, k, rows], s [B, H, k / 32, rows]
        t3, s3 = t.contiguous().view(BH, k, rows), s.contiguous().view(BH, k // 32, rows)
        return mx_gemm._pack(t3, s3, fid, 32, BH, rows, k, (k * rows, 1, rows), (s3.stride(0), 1, s3.stride(1)), check=False)

    pq = mx_operand.operand(q, mx_operand.ROWS, fid, 32, BH * Q, D)
    if pq is None:
        q3, s3 = q.contiguous().view(BH, Q, D), q_scale.contiguous().view(BH, Q, D // 32)
        pq = mx_gemm._pack(q3, s3, fid, 32, BH, Q, D, (Q * D, D, 1), (s3.stride(0), s3.stride(1), 1), check=False)
    pk = mx_operand.operand(kT, mx_operand.SECOND, fid, 32, BH * C, D) or second(kT, kT_scale, C, D)
    pv = mx_operand.operand(v, mx_operand.SECOND, fid, 32, BH * D, C) or second(v, v_scale, D, C)
    return pq, pk, pv


def launch_mxf(fid, packed, mask, mask_strides, scaling, scaling_is_div, p_qmap, p_quant_max, out, block_size=32):
    """qt_attention_mxf on packed operands into `out` [B, H, Q, D] bf16.  Returns the status code."""
    pq, pk, pv = packed
    B, H, Q, D = out.shape
    C = pk[0].numel() // (B * H * mx_operand.row_bytes(D, fid))
    return _native.lib().qt_attention_mxf(
        pq[0].data_ptr(), pq[1].data_ptr(), pk[0].data_ptr(), pk[1].data_ptr(), pv[0].data_ptr(), pv[1].data_ptr(),
        mask.data_ptr() if mask is not None else None, *mask_strides, float(scaling), int(bool(scaling_is_div)), fid, p_qmap.data_ptr(),
        float(p_quant_max), out.data_ptr(), B, H, Q, C, D, block_size, _stream_ptr(out))
