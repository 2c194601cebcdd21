"""The outlier side path of a block-scaled linear layer on the device (upstream decomposed.py:450-566).

An activation spec with `outlier=` lowers to filter_outlier -> quantize_mx -> linear_mx plus spmm_csr on the outliers
(quantize_pt2e.py:299-304, 393-412).  The two outlier operators run as kernels of csrc/qt_outlier.hip:

  filter_outlier   qt_filter_outlier_*: three launches (inlier + row counts, a one-workgroup scan, compaction), all four results of
                   static shape, no host read;
  spmm_csr         qt_spmm_csr_*: one launch that takes the stored weight -- [N, K] or [K, N], codes, block scales -- in place,
                   accumulates in fp32 in a fixed order (the row's entries, in groups of 16) and rounds once.  Deterministic, unlike
                   the composite's index_add_, and more accurate than its per-step rounding in bf16.

Governed by QT_MX_GEMM like linear_mx / matmul_mx / conv2d_mx, counted in this module's own STATS.  Anything the kernels do not take
returns None and the caller runs the composite unchanged.

Eager calls keep the composite's behaviour towards a truncated CSR at the cost of one 4-byte read of indptr[-1] AFTER the launches:
filter_outlier logs the truncation warning, spmm_csr raises the IndexError.  While the current stream is capturing neither read
happens; the kernels clamp every row's range to the arrays' capacity, so a truncated CSR is memory-safe there and its stored entries
are the ones multiplied."""
import logging

import torch

from . import _native, switches
from .fake_quantize import _stream_ptr

__all__ = ["filter_outlier_or_none", "spmm_csr_or_none", "STATS"]

_LIMIT = 2 ** 31 - 1          # rows, columns, element counts the kernels index with int32 results
_CODE_MAX = 256               # codebook entries qt_spmm_csr_* keeps in LDS
_DTYPES = (torch.bfloat16, torch.float32)


class _Stats:
    """How many outlier operators took the kernels / the composite on device tensors (tests assert on it)."""
    def __init__(self):
        self.native = 0
        self.fallback = 0

    def reset(self):
        self.native = self.fallback = 0


STATS = _Stats()
_DEBUG = False            # set outlier._DEBUG = True to print why a call took the composite


def _fallback(why):
    STATS.fallback += 1
    if _DEBUG:
        print("outlier: composite:", why, flush=True)
    return None


def _on_device(t):
    """A real device tensor: not a CPU or meta tensor, and not the fake / functional stand-in of a trace (no storage to hand to a kernel)."""
    return (t.device.type == "cuda" and type(t) in (torch.Tensor, torch.nn.Parameter) and not torch._is_functional_tensor(t))


def _capturing():
    return torch.cuda.is_current_stream_capturing()


def _rounded_to(dtype, value):
    """`value` as torch's `tensor > value` sees it: the Python scalar takes the tensor's dtype."""
    return float(torch.tensor(float(value), dtype=torch.float64).to(dtype))


def _filter_why_not(input, max_nnz):
    if input.dtype not in _DTYPES:
        return f"dtype {input.dtype}"
    if input.dim() < 1 or input.numel() == 0:
        return f"shape {tuple(input.shape)}"
    if input.numel() >= _LIMIT:
        return f"{input.numel()} elements"
    if not 0 <= max_nnz <= input.numel():
        return f"max_nnz {max_nnz}"
    return None


def filter_outlier_or_none(input, threshold, max_pct=0.05):
    """filter_outlier through qt_filter_outlier_* -> (inlier, data, indices, indptr), or None.  A non-contiguous input is made contiguous."""
    if not _on_device(input):
        return None
    if not switches.on("QT_MX_GEMM"):
        return _fallback("QT_MX_GEMM=0")
    max_nnz = int(input.numel() * max_pct)
    why = _filter_why_not(input, max_nnz)
    if why is not None:
        return _fallback(why)
    x = input.contiguous()
    cols = x.shape[-1]
    rows = x.numel() // cols
    inlier = torch.empty_like(x)
    data = torch.empty((max_nnz,), dtype=x.dtype, device=x.device)
    indices = torch.empty((max_nnz,), dtype=torch.int32, device=x.device)
    indptr = torch.empty((rows + 1,), dtype=torch.int32, device=x.device)
    L = _native.lib()
    fn = L.qt_filter_outlier_bf16 if x.dtype == torch.bfloat16 else L.qt_filter_outlier_f32
    rc = fn(x.data_ptr(), inlier.data_ptr(), data.data_ptr() if max_nnz else None, indices.data_ptr() if max_nnz else None,
            indptr.data_ptr(), rows, cols, _rounded_to(x.dtype, threshold), max_nnz, _stream_ptr(x))
    if _native.declined(rc):
        return _fallback(f"qt_filter_outlier declined (code {rc})")
    _native.check(rc, "qt_filter_outlier")
    STATS.native += 1
    if not _capturing():
        nnz = int(indptr[-1])
        if nnz > max_nnz:
            logging.getLogger(__package__ + ".decomposed").warning(
                f"Number of non-zero elements {nnz} exceeds max_nnz {max_nnz}, truncating.")
    return inlier, data, indices, indptr


def _scale_view(B, scale, block_size):
    """(rows, cols, div0, div1) of the block scale as expand(scale, B.shape, block_size) reads it, or a reason (str)."""
    if scale.dim() > 2:
        return f"scale of {scale.dim()} dimensions"
    if isinstance(block_size, bool) or not isinstance(block_size, int) or block_size < 1:
        return f"block size {block_size!r}"
    shape = (1,) * (2 - scale.dim()) + tuple(scale.shape)
    divs = []
    for s, d in zip(shape, B.shape):
        div = 1 if s == d else block_size
        if s < 1 or s * div < d:
            return f"scale {tuple(scale.shape)} does not cover B {tuple(B.shape)} in blocks of {block_size}"
        divs.append(div)
    return shape[0], shape[1], divs[0], divs[1]


def _spmm_why_not(data, indices, indptr, B, B_scale, B_code, block_size):
    others = [t for t in (indices, indptr, B, B_scale, B_code) if t is not None]
    if not all(_on_device(t) and t.device == data.device for t in others):
        return "operands that are not tensors of one device"
    if data.dtype not in _DTYPES:
        return f"dtype {data.dtype}"
    if B.dtype != data.dtype or (B_scale is not None and B_scale.dtype != data.dtype) or (B_code is not None and B_code.dtype != data.dtype):
        return (f"dtypes: data {data.dtype}, B {B.dtype}, scale {None if B_scale is None else B_scale.dtype}, "
                f"codebook {None if B_code is None else B_code.dtype}")
    if indices.dtype != torch.int32 or indptr.dtype != torch.int32:
        return f"indices {indices.dtype}, indptr {indptr.dtype}"
    if data.dim() != 1 or indices.dim() != 1 or indptr.dim() != 1 or B.dim() != 2 or indices.numel() < data.numel():
        return f"shapes: data {tuple(data.shape)}, indices {tuple(indices.shape)}, indptr {tuple(indptr.shape)}, B {tuple(B.shape)}"
    if indptr.numel() < 2 or B.numel() == 0:
        return "an empty product"
    if max(indptr.numel(), data.numel(), B.shape[0], B.shape[1]) >= _LIMIT:
        return "a dimension of 2^31 - 1 or more"
    if B_code is not None and (B_code.dim() != 1 or not 1 <= B_code.numel() <= _CODE_MAX):
        return f"a codebook of shape {tuple(B_code.shape)}"
    if B_scale is not None:
        view = _scale_view(B, B_scale, block_size)
        if isinstance(view, str):
            return view
    return None


def spmm_csr_or_none(data, indices, indptr, B, B_scale=None, B_code=None, block_size=None, weight_transposed=False):
    """spmm_csr through qt_spmm_csr_* -> Y [rows, N] in data's dtype, or None.  Non-contiguous operands are made contiguous (the CSR
    arrays and the scale are small; a strided weight is the one case that costs a copy)."""
    if not _on_device(data):
        return None
    if not switches.on("QT_MX_GEMM"):
        return _fallback("QT_MX_GEMM=0")
    why = _spmm_why_not(data, indices, indptr, B, B_scale, B_code, block_size)
    if why is not None:
        return _fallback(why)
    data, indices, indptr, B = data.contiguous(), indices.contiguous(), indptr.contiguous(), B.contiguous()
    M = indptr.numel() - 1
    N, K = (B.shape[1], B.shape[0]) if weight_transposed else (B.shape[0], B.shape[1])
    scale = code = None
    srows = scols = div0 = div1 = 0
    if B_scale is not None:
        scale = B_scale.contiguous()
        srows, scols, div0, div1 = _scale_view(B, B_scale, block_size)
    if B_code is not None:
        code = B_code.contiguous()
    cap = data.numel()
    Y = torch.empty((M, N), dtype=data.dtype, device=data.device)
    L = _native.lib()
    fn = L.qt_spmm_csr_bf16 if data.dtype == torch.bfloat16 else L.qt_spmm_csr_f32
    rc = fn(data.data_ptr() if cap else None, indices.data_ptr() if cap else None, indptr.data_ptr(), cap, M, B.data_ptr(), N, K,
            int(bool(weight_transposed)), scale.data_ptr() if scale is not None else None, srows, scols, div0, div1,
            code.data_ptr() if code is not None else None, code.numel() if code is not None else 0, Y.data_ptr(), _stream_ptr(data))
    if _native.declined(rc):
        return _fallback(f"qt_spmm_csr declined (code {rc}): K = {K}")
    _native.check(rc, "qt_spmm_csr")
    STATS.native += 1
    if not _capturing():
        nnz = int(indptr[-1])
        if nnz > cap:                                             # the truncated case: upstream's loop runs off the arrays
            raise IndexError(f"index {cap} is out of bounds for dimension 0 with size {cap}")
    return Y
