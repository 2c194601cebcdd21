"""The block-scaled operand hand-over: how quantize / quantize_mx tell linear_mx / matmul_mx / conv2d_mx what their results hold, and
the facts about the kernels both sides need.  The record is Python attributes on the tensors (handover.py is the same protocol for
the per-tensor FP8 path):

  _qt_mx_ver            the tensor's `_version` when the other attributes were written; anything else means stale
  _qt_dtype             on a value map: the name of the format it rounds to ("" = looked at, none this package knows)
  _qt_mx_fmt            on quantized values: the name of the format they are in (any name; consumers test `in FMT_ID`)
  _qt_pow2              on a block scale: a power of two by construction
  _qt_mx_packed_act, _qt_mx_packed_b, _qt_mx_packed_nhwc
                        on quantized values: (format id, block size, codes, e8m0), the packed operand of the matrix instruction;
                        the name says which logical rows the code rows are (the layouts ROWS, SECOND, NHWC below)
  _qt_mx_packed, _qt_mx_packed_conv
                        on a weight: (key, (format id, codes, e8m0) or None), the packed constant operand of the GEMM / the
                        convolution.  The key carries both version counters, so these two need no stamp.
  _qt_mxi_packed        on a weight: (key, (codes int8, scales fp32) or None), its operand in the integer family (qt_mxi_gemm); the
                        key carries the version counters of weight, scale and codebook
  _qt_mxi_code          on a codebook: (version, whether the integer GEMM takes it): one host read per codebook

`_qt_mx_fmt` also names the integer formats (INT_BITS): `quantize` with a block size and `quantize_mx` write it for an integer map
whatever the scales are (quantized_int), and the integer route of mx_gemm.py reads it (int_format_of).

This module is the only code that reads or writes them.  A stale record reads as no record at all -- the format too, not only the
operand: a consumer that still believed the format would pack the modified values without the packer's check.  Inference tensors
(made under torch.inference_mode()) have no version counter: their stamp is "untracked", the record always counts as valid, and a
write in place CANNOT be seen there.  It imports torch and, to compare a map by content, fake_quantize's tables; no routing."""
import torch

# ---- what the kernels take (csrc/qt_mx_tile.h) -----------------------------------------------------------------------------------
FMT_ID = {"fp8_e4m3": 0, "fp8_e5m2": 1, "fp6_e2m3": 2, "fp6_e3m2": 3, "fp4_e2m1": 4}
BITS = {0: 8, 1: 8, 2: 6, 3: 6, 4: 4}
PAIRS = {(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (2, 4), (3, 4)}      # (first, second) operand format ids
NARROW_FIRST = ("fp4_e2m1", "fp6_e2m3", "fp6_e3m2", "fp8_e4m3", "fp8_e5m2")


def row_bytes(k, fid):
    """Bytes of a code row of `k` elements in format `fid`."""
    return k * BITS[fid] // 8


def row_is_whole_chunks(k, fid):
    """The kernels fetch code rows in 16-byte chunks: a row has to be a whole number of them."""
    return row_bytes(k, fid) % 16 == 0


# ---- the integer family (qt_mxi_pack / qt_mxi_gemm): int8 codes, fp32 block scales of any value ----------------------------------
INT_BITS = {f"int{n}": n for n in range(2, 9)}       # format name -> N: every value is an integer in [-2^(N-1), 2^(N-1) - 1]
INT_BLOCKS = (32, 64, 128)
INT_CODEBOOK_MAX = 256


# ---- the layouts of a packed operand, and the stamp --------------------------------------------------------------------------------
ROWS = "rows"         # code rows = rows of the tensor as stored: the first operand of linear_mx / matmul_mx
SECOND = "second"     # code rows = the [batch N, K] second operand of matmul_mx of a [..., K, N] tensor
NHWC = "nhwc"         # code rows = the pixels of an [N, C, H, W] tensor, channels innermost: conv2d_mx's activation
_OPERAND = {ROWS: "_qt_mx_packed_act", SECOND: "_qt_mx_packed_b", NHWC: "_qt_mx_packed_nhwc"}
_FIELDS = ("_qt_dtype", "_qt_mx_fmt", "_qt_pow2") + tuple(_OPERAND.values())


def _version(t):
    return "untracked" if t.is_inference() else t._version


def valid(t):
    return getattr(t, "_qt_mx_ver", None) == _version(t)


def _write(t, name, value):
    """Every writer ends here.  What an earlier, now stale stamp vouched for goes first, so that the new stamp does not revive it."""
    if not valid(t):
        forget(t)
    setattr(t, name, value)
    t._qt_mx_ver = _version(t)
    return t


def _read(t, name):
    return getattr(t, name, None) if valid(t) else None


def forget(t):
    """Drops the whole record."""
    for name in _FIELDS + ("_qt_mx_ver",):
        t.__dict__.pop(name, None)
    return t


# ---- the map tag -------------------------------------------------------------------------------------------------------------------
def tag_map(qmap, name):
    """The identity map of "no format" (dtype None) is tagged "None": from the reader, None means no tag."""
    return _write(qmap, "_qt_dtype", "None" if name is None else name)


def map_name(qmap):
    """The name a value map was tagged with, while nothing was written to the map since; else None."""
    return _read(qmap, "_qt_dtype")


def format_of_qmap(qmap):
    """Name of the native element format a value map rounds to, or None.  The answer is kept on the tensor object (module buffers
    are long-lived objects; a cache keyed by address would go stale when memory is re-used)."""
    name = map_name(qmap)
    if name is None:
        from .fake_quantize import _table_for
        name = ""
        if qmap.numel() == 65536 and qmap.dtype == torch.bfloat16:
            bits = qmap.view(torch.int16)
            for cand in FMT_ID:
                if torch.equal(bits, _table_for(cand, qmap.device).view(torch.int16)):       # host sync, once per buffer
                    name = cand
                    break
        tag_map(qmap, name)
    return name if name in FMT_ID else None


def int_format_of_qmap(qmap):
    """Name of the integer format (INT_BITS) a value map was tagged with, or None.  By tag alone: a map without one is not compared
    by content against the integer tables."""
    name = map_name(qmap)
    return name if name in INT_BITS else None


# ---- values and scales -------------------------------------------------------------------------------------------------------------
def set_format(values, name):
    return _write(values, "_qt_mx_fmt", name)


def format_of(values):
    return _read(values, "_qt_mx_fmt")


def quantized_int(values, qmap):
    """The tail of every quantize / quantize_mx route without zero points, kernel or composite, on any device and whatever the
    scales are: values rounded with an integer map remember its name.  Returns whether they do."""
    name = int_format_of_qmap(qmap) if values is not None else None
    if name is not None:
        set_format(values, name)
    return name is not None


def int_format_of(values):
    """The integer format `values` remember, or None."""
    name = format_of(values)
    return name if name in INT_BITS else None


def int_codebook_ok(code):
    """Whether a codebook is one the integer GEMM takes: at most 256 entries, all integers in [-128, 127].  One host read per
    codebook, kept on the tensor object with its version (a codebook written in place is read again)."""
    stamp = _version(code)
    hit = code.__dict__.get("_qt_mxi_code")
    if hit is not None and hit[0] == stamp:
        return hit[1]
    ok = code.dim() == 1 and 1 <= code.numel() <= INT_CODEBOOK_MAX and code.is_floating_point()
    if ok:
        c = code.detach().double()
        ok = bool(((c == c.trunc()) & (c >= -128) & (c <= 127)).all())           # host sync on a device codebook
    code._qt_mxi_code = (stamp, ok)
    return ok


def set_pow2(scale):
    return _write(scale, "_qt_pow2", True)


def is_pow2(scale):
    return bool(_read(scale, "_qt_pow2"))


def set_operand(values, layout, fid, block_size, codes, e8):
    return _write(values, _OPERAND[layout], (fid, block_size, codes, e8))


def operand_record(values, layout):
    """(format id, block size, codes, e8m0) as the producer left it under `layout`, or None."""
    return _read(values, _OPERAND[layout])


def operand(values, layout, fid, block_size, rows, k):
    """The one look-up: (codes, e8m0) when `values` carries the operand of `layout` in this format, block size and extent."""
    rec = operand_record(values, layout)
    if rec is not None and rec[0] == fid and rec[1] == block_size and rec[2].shape == (rows, row_bytes(k, fid)):
        return rec[2], rec[3]
    return None


def drop_operand(values):
    """Forgets the packed operand, under every layout, and keeps format and flag: the consumer then packs the values itself."""
    for name in _OPERAND.values():
        values.__dict__.pop(name, None)
    return values


def quantized(values, scale, fmt_name, layout=None, fid=-1, block_size=None, codes=None, e8=None):
    """The tail of a quantize_mx kernel that wrote power-of-two scales: flag, format (when the map has one) and operand (when the
    kernel wrote its codes)."""
    set_pow2(scale)
    if fmt_name is not None:
        set_format(values, fmt_name)
    if codes is not None:
        set_operand(values, layout, fid, block_size, codes, e8)


def carry(src, src_scale, view, view_scale):
    """`view` / `view_scale` are views of `src` / `src_scale` (same storage, same version counter): flag and format hold for them as
    they stand, and the source's ROWS operand is the view's under the layout this returns -- SECOND for transpose(-1, -2), NHWC for
    permute(0, 3, 1, 2); None when no operand was carried."""
    if is_pow2(src_scale):
        set_pow2(view_scale)
    if format_of(src) is not None:
        set_format(view, format_of(src))
    rec = operand_record(src, ROWS)
    layout = None
    if rec is not None:
        if src.dim() >= 2 and _same_view(view, src.transpose(-1, -2)):
            layout = SECOND
        elif src.dim() == 4 and _same_view(view, src.permute(0, 3, 1, 2)):
            layout = NHWC
        if layout is not None:
            set_operand(view, layout, *rec)
    return layout


def _same_view(a, b):
    return a.shape == b.shape and a.stride() == b.stride() and a.data_ptr() == b.data_ptr()


def copy_hints(src, dst):
    """`dst` is a fresh copy of `src`'s values: map tag, format and flag go along, stamped for the copy (the packed operand does not)."""
    for name in ("_qt_dtype", "_qt_pow2", "_qt_mx_fmt"):
        value = _read(src, name)
        if value is not None:
            _write(dst, name, value)
    return dst


# ---- the constant operand ----------------------------------------------------------------------------------------------------------
GEMM_SLOT, CONV_SLOT = "_qt_mx_packed", "_qt_mx_packed_conv"


def weight_operand(weight, scale, block_size, slot, as_rows, extent, pack):
    """A weight's packed operand, (format id, codes, e8m0) or None when the packer refuses it in every format: packed once, cached on
    the tensor object under `slot`.  as_rows() -> (weight, scale) as contiguous [rows, K] / [rows, K / block]; `extent` is what the
    16-byte rule applies to; pack(w, s, fid, block_size) -> (codes, e8m0) or None with the packer's check on.  A weight of a
    remembered format is tried in that format alone, any other narrow-first."""
    key = (weight._version, scale.data_ptr(), scale._version, block_size)
    hit = getattr(weight, slot, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    w, s = as_rows()
    known = format_of(weight)
    result = None
    for name in ((known,) if known in FMT_ID else NARROW_FIRST):
        fid = FMT_ID[name]
        if not row_is_whole_chunks(extent, fid):
            continue
        packed = pack(w, s, fid, block_size)
        if packed is not None:
            result = (fid, packed[0], packed[1])
            break
    setattr(weight, slot, (key, result))
    return result


INT_SLOT = "_qt_mxi_packed"


def int_weight_operand(weight, scale, code, block_size, pack):
    """A weight's operand in the integer family, (codes int8, scales fp32) or None when the packer's check refuses it: packed once,
    cached on the tensor object under its own slot (the float family's GEMM_SLOT is another cache).  pack() -> (codes, scales) or
    None, with the check on.  The key carries the version counters of weight, scale and codebook."""
    key = (weight._version, scale.data_ptr(), scale._version, block_size,
           None if code is None else (code.data_ptr(), code._version))
    hit = getattr(weight, INT_SLOT, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    result = pack()
    setattr(weight, INT_SLOT, (key, result))
    return result

