"""The producer-to-consumer hand-over: how a producing kernel (RMSNorm, LayerNorm, GELU, SiLU * up, rotary, the one-launch MLP, a
fake-quantizer's own pass) tells the consumer of its result what it already did.  The record is Python attributes on the result tensor:

  _qt_ver               the tensor's `_version` when the other attributes were written; anything else means stale
  _qt_fq_done_by        the fake-quantizer whose call the producer already evaluated
  _qt_also_done         [(fq, codes)]: further fake-quantizers evaluated in the same launch
  _qt_fp8               FP8 codes of the fake-quantized values
  _qt_fp8_of_transpose  the same, on the K^T view
  _qt_lazy              only the codes were written; the bf16 storage is unwritten (NaN under QT_LAZY_POISON=1)
  _qt_origin            tensor_key of the tensor this one is fq(.) of (sibling GEMMs)

This module is the only code that reads or writes them.  It imports nothing from the package.  (mx_operand.py is the same protocol
for the block-scaled operands of linear_mx / matmul_mx / conv2d_mx.)"""
import weakref

import torch

from . import switches


def valid(t):
    """The record is stamped with the tensor's version counter: an in-place modification in between (a user forward hook, `add_`)
    makes it stale, and the consumer then does its own pass."""
    return getattr(t, "_qt_ver", None) == t._version


def tensor_key(t):
    """Identity of a tensor's current contents: same storage address, no in-place write since, same extent."""
    return (t.data_ptr(), t._version, tuple(t.shape))


def fp8_view(t8, fmt):
    """uint8 codes as the torch FP8 dtype of `fmt` (a QtFormat, or a fake-quantizer carrying one): E5M2 exactly when p0 == 2."""
    fmt = getattr(fmt, "_qt_format", fmt)
    return t8.view(torch.float8_e5m2 if fmt.p0 == 2 else torch.float8_e4m3fn)


def stamp(t, done_by=None, codes=None, also=None, origin=None, lazy=False, register=True):
    """The one writer: records the fields given and `_qt_ver`, once and last.  lazy: the bf16 values were not written (mark_lazy);
    register=False sets the flag alone -- no poison, no registry, so a view of `t` is not recognised by materialize -- which is what
    rope_fq's value-job branch and pt2e_fusion.PreparedAttention have always done."""
    if done_by is not None:
        t._qt_fq_done_by = done_by
    if codes is not None:
        t._qt_fp8 = codes
    if also is not None:
        t._qt_also_done = also
    if origin is not None:
        t._qt_origin = origin
    if lazy and register:
        mark_lazy(t)
    elif lazy:
        t._qt_lazy = True
    t._qt_ver = t._version
    return t


def _field(t, name, unchecked=False):
    return getattr(t, name, None) if unchecked or valid(t) else None


def codes(t, unchecked=False):
    """The checked readers: the field when the record is valid, else None.  `unchecked` reads it whatever the version counter says;
    the few sites that always did so say it in a comment."""
    return _field(t, "_qt_fp8", unchecked)


def done_by(t, unchecked=False):
    return _field(t, "_qt_fq_done_by", unchecked)


def origin(t, unchecked=False):
    return _field(t, "_qt_origin", unchecked)


def also_done(t):
    return _field(t, "_qt_also_done")


def codes_of_transpose(t):
    return _field(t, "_qt_fp8_of_transpose")


def carry(X, x8, src):
    """The result of a fake-quantizer's call on `src` when X already holds fq(src), value for value: a view of X (in src's shape)
    carrying this call's codes and `src`'s key as origin.  If X's values were never written the view's are not either: it inherits
    the flag (alone: X itself is the registered tensor)."""
    return stamp(X.view(src.shape), codes=x8, origin=tensor_key(src), lazy=is_lazy(X), register=False)


def transposed(key, key_t):
    """key_t = a transposed view of key (it shares the version counter).  Fake-quant is elementwise: done for K means done for K^T,
    and the codes of K itself ([B, H, S, D], contiguous) travel along under their own name.  Nothing when key's record is stale."""
    if done_by(key) is not None:
        key_t._qt_fq_done_by = key._qt_fq_done_by
        if codes(key) is not None:
            key_t._qt_fp8_of_transpose = key._qt_fp8
        key_t._qt_ver = key._qt_ver
    return key_t


# ---- codes-only results ---------------------------------------------------------------------------------------------------------
_LAZY = {}          # data_ptr -> weakref of a tensor whose values were not written (its FP8 codes were): views of it lose the attribute


def is_lazy(t):
    return t.__dict__.get("_qt_lazy", False)


def unwritten(shape=None, dtype=None, device=None, like=None, out=None):
    """The one allocator of a tensor that is handed to its reader BEFORE the launch that writes it has been issued: torch.empty of the
    shape triple (or `like` a tensor; or `out`, a tensor the caller already allocated), filled with NaN under QT_LAZY_POISON=1 (the
    tests), so that a read that comes too early cannot go unnoticed."""
    if out is None:
        out = torch.empty_like(like) if like is not None else torch.empty(shape, dtype=dtype, device=device)
    if switches.on("QT_LAZY_POISON"):
        out.fill_(float("nan"))
    return out


def mark_lazy(t):
    """t's values were not written (its FP8 codes were): it is poisoned as every unwritten tensor is, so that a read that bypasses
    materialize cannot go unnoticed.  t is registered by its address so that a VIEW of it -- a reshape between the producer and the
    consuming hook drops Python attributes -- is still recognised by materialize; the entry dies with the tensor."""
    stamped = valid(t)
    unwritten(out=t)
    if stamped:
        t._qt_ver = t._version                        # (the fill is not a modification of the result the hand-over describes)
    t._qt_lazy = True
    ptr = t.data_ptr()
    _LAZY[ptr] = weakref.ref(t)
    weakref.finalize(t, lambda p=ptr: _LAZY.pop(p, None) if (_LAZY.get(p) is not None and _LAZY[p]() is None) else None)
    return t


def lazy_owner(t):
    """The registered lazy tensor that `t` is a view of (same storage, same extent), or None."""
    if not _LAZY:
        return None
    ref = _LAZY.get(t.data_ptr())
    base = ref() if ref is not None else None
    if (base is not None and base is not t and is_lazy(base) and base.device == t.device and base.dtype == t.dtype
            and base.numel() == t.numel() and t.is_contiguous()):
        return base
    return None


def materialize(t):
    """A producer that knew its consumer multiplies FP8 codes wrote ONLY the codes of fq(t).  The fake-quantized values are exactly
    what the codes decode to, so whoever asks for them after all gets them here."""
    if is_lazy(t):
        t.copy_(t._qt_fp8.to(t.dtype))
        t._qt_lazy = False
        t._qt_ver = t._version
        return
    base = lazy_owner(t)
    if base is not None:
        # a view of a lazy tensor: decode through the owner
        stamped = valid(t)
        materialize(base)
        if stamped:
            t._qt_ver = t._version
