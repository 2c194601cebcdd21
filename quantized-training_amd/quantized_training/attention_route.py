"""Routing of the inference attention core (no gradients), for the module path (modules/quantizable/attention.py) and the PT2E path
(pt2e_fusion.py).  fused_attention_or_none: the whole core as qt_attention_fp8 (_attention_fp8_or_none), else table_format_core
(qt_attention_rows_bf16, else the two-pass qt_attention_fq*_bf16 in its three entry points).  fused_scores_to_probs_or_none, behind a
library Q.K^T: the score pass + library FP8 P.V, else the softmax pass + torch's P.V.  A route that does not apply returns None and the
caller goes on to the next; all are device paths.  The additive mask travels as ONE AttentionMask; the value pass a rotary launch wrote
ahead of the core's call is a precomputed.Slot (VALUE_CODES_T, VALUE_T_ROWS)."""
import ctypes

import torch

from . import _native, handover, planner_checks as pc, precomputed, switches
from .fake_quantize import STATS, FusedAmaxObsFakeQuantize, _launch_format, _stream_ptr, launch_scale_update
from .fused import _IDENTITY, _LT, lt_fp8_gemm


class AttentionMask:
    """A broadcastable additive bf16 mask as the kernels consume it in place: `view` (the mask sliced to the key count; None without a
    mask), `ptr` (its address, or None), `strides` (elements, for (b, h, q); 0 where the mask broadcasts) and `owner` -- the tensor object
    the attention block was handed, of which `view` is a view."""
    __slots__ = ("view", "ptr", "strides", "owner")

    def __init__(self, view, strides, owner):
        self.view, self.strides, self.owner = view, strides, owner
        self.ptr = view.data_ptr() if view is not None else None

    @classmethod
    def of(cls, attention_mask, B, H, Q, C, device, align, no_grad=False):
        """The descriptor, or None if the mask cannot be consumed in place (no_grad: or requires grad -- the training launches return
        no mask gradient).  No mask: a null pointer and zero strides."""
        if attention_mask is None:
            return cls(None, (0, 0, 0), None)
        m = attention_mask[..., :C]
        if m.dtype != torch.bfloat16 or m.dim() != 4 or m.stride(-1) != 1 or m.device != device or (no_grad and m.requires_grad):
            return None
        if m.shape[0] not in (1, B) or m.shape[1] not in (1, H) or m.shape[2] not in (1, Q):
            return None
        sb = m.stride(0) if m.shape[0] == B and B > 1 else 0
        sh = m.stride(1) if m.shape[1] == H and H > 1 else 0
        sq = m.stride(2) if m.shape[2] == Q and Q > 1 else 0
        if (sb | sh | sq) % align != 0 or m.data_ptr() % (2 * align) != 0:
            return None
        return cls(m, (sb, sh, sq), attention_mask)

    def row_live(self, B, H, Q, C, st):
        """(row_live_ptr, stride_b, stride_h, stride_q, irregular_ptr): the per-row extent of the unmasked part of the mask
        (qt_mask_row_live_checked) with its strides in rows; all null without a mask or when its rows are not evenly spaced.  The scan
        is kept as an attribute of `owner`: the cached causal mask of a window evaluation is the same object for every layer and window,
        a mask Hugging Face builds per forward is the same object for every layer of that forward; a new object (or a new version of
        it) is scanned again.  The scan also leaves, behind the extents (irregular_ptr), whether any row is NOT exactly "zeros, then the
        dtype's minimum" (0: none, and the mask is not read): the kernels read that on the device (no host read-back: also inside a
        stream capture)."""
        mask = self.view
        if mask is None:
            return None, 0, 0, 0, None
        mb, mh, mq, _ = mask.shape
        rs = mask.stride(2) if mq > 1 else C
        if (mh > 1 and mask.stride(1) != mq * rs) or (mb > 1 and mask.stride(0) != mh * mq * rs) or rs < C:
            return None, 0, 0, 0, None
        rows = mb * mh * mq
        key = (self.ptr, self.owner._version, tuple(mask.shape), mask.stride())
        hit = getattr(self.owner, "_qt_row_live", None)
        if hit is not None and hit[0] == key:
            rl = hit[1]
        else:
            rl = torch.empty(rows + 1, dtype=torch.int32, device=mask.device)
            _native.check(_native.lib().qt_mask_row_live_checked(self.ptr, rows, C, rs, rl.data_ptr(), rl.data_ptr() + 4 * rows, st),
                          "qt_mask_row_live_checked")
            self.owner._qt_row_live = (key, rl)
        return (rl.data_ptr(), (mh * mq if mb == B and B > 1 else 0), (mq if mh == H and H > 1 else 0), (1 if mq == Q and Q > 1 else 0),
                rl.data_ptr() + 4 * rows)


def readable_in_place(t):
    """May the kernels read this strided [B, H, S, D] bf16 view where it lies: last stride 1, the other strides multiples of 8 elements,
    a 16-byte-aligned base."""
    return t.dtype == torch.bfloat16 and t.stride(-1) == 1 and not any(s % 8 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0


def fp8_codes_of_view(t, fq, st):
    """The FP8 codes of fq(t), contiguous, for a readable_in_place view `t` and a stateless FP8 `fq`.  The caller counts the call."""
    B, H, rows, D = t.shape
    t8 = torch.empty((B, H, rows, D), dtype=torch.uint8, device=t.device)
    _native.check(_native.lib().qt_fake_quant_rows_bf16_fp8(t.data_ptr(), None, t8.data_ptr(), B, H, rows, D, t.stride(0), t.stride(1), t.stride(2),
                                                            ctypes.byref(fq._qt_format), st), "qt_fake_quant_rows_bf16_fp8")
    return t8


def count_call(fq, numel):
    """A call of `fq` that a launch evaluated, counted as its own forward would count it."""
    fq.__dict__["_qt_calls"] = fq.__dict__.get("_qt_calls", 0) + 1
    STATS.add(numel)


def _probs_fq_launch_args(fq_p, device, st, numel, drop_unit_scale=False):
    """(fmt, lut, scale_ptr, amax_ptr) with which a softmax / attention launch applies the probabilities' fake-quantizer, after this call's
    bookkeeping in this order: _move_to, the first call's history resize, the scale update, STATS.add(numel).  No or a switched-off
    fake-quantizer: the identity format, nothing touched.  drop_unit_scale: no scale pointer for a stateless format whose scale is one."""
    if fq_p is None or not (fq_p._observe or fq_p._quantize):
        return _IDENTITY, None, None, None
    fq_p._move_to(device)
    fmt = fq_p._qt_format if fq_p._quantize else _IDENTITY
    if fq_p._observe:
        if fq_p.amax_history.numel() == 0:
            fq_p.amax_history.resize_((fq_p.amax_history_len,)).fill_(0.0)
            fq_p.scale.resize_(()).fill_(1.0)
        launch_scale_update(fq_p.amax_history, fq_p.scale, fq_p.quant_max, fq_p.force_scale_power_of_two, st)
    lut = None
    if fmt.kind == _native.QT_FMT_LUT:
        fmt = _launch_format(fmt, fq_p.qmap)             # the row form of the map where the allocation carries it
        lut = fq_p.qmap.data_ptr()
    unit_scale = drop_unit_scale and fq_p.qscheme is None and getattr(fq_p, "_scale_is_one", True)      # no scale tensor at all
    scale_ptr = fq_p.scale.data_ptr() if (fq_p._quantize and not unit_scale) else None
    amax_ptr = fq_p.amax_history.data_ptr() if fq_p._observe else None
    STATS.add(numel)
    return fmt, lut, scale_ptr, amax_ptr


def fused_scores_to_probs_or_none(attn, scores, attention_mask, scaling, dropout, value):
    """scale -> +mask -> softmax -> fake-quant(probabilities) in ONE HIP pass (qt_softmax_fq_bf16), then
    av_matmul on the quantized probabilities.  Applies when nothing observes the intermediate tensors:
    `attn_scaling` and `softmax` carry no activation hooks (the `--quantize_forward gemm` default), no
    dropout is active, bf16 device tensors, and av_matmul's per-tensor fake-quantizers already exist
    (they are created by the first, unfused, call).  Returns (probs_q, attn_output) or None."""
    if not switches.on("QT_FUSED_SOFTMAX"):
        return None
    if not (scores.device.type == "cuda" and scores.dtype == torch.bfloat16 and scores.dim() == 4):
        return None
    if torch.is_grad_enabled() and scores.requires_grad:
        return None
    if dropout and attn.training:
        return None
    if getattr(attn.attn_scaling, "activation_pre_process", None) is not None or getattr(attn.softmax, "activation_pre_process", None) is not None:
        return None
    # (their forward hooks only, where fused_attention_or_none also refuses pre-hooks on the first two: kept as found, no reason found)
    if not (pc.no_output_hook(attn.attn_scaling) and pc.no_output_hook(attn.softmax) and pc.no_output_hook(attn.av_matmul)):
        return None
    holder = getattr(attn.av_matmul, "activation_pre_process", None)
    fq_p = fq_v = None
    if holder is not None:
        fqs = pc.holder_fqs(attn.av_matmul, "activation_pre_process", "0", "1", exact=False)
        if fqs is None:
            return None                       # first call: let the hook create them
        fq_p, fq_v = fqs
        if not pc.plain_per_tensor(fq_p):
            return None
    # (AT MOST quantize()'s one pre-hook, where the other planners ask for exactly one: a holder without its hook passes here)
    if not pc.hook_counts(attn.av_matmul, forward_pre=(0, 1) if holder is not None else 0):
        return None
    B, H, Q, C = scores.shape
    if C % 8 != 0 or C > 4096 or not scores.is_contiguous():
        return None
    mk = AttentionMask.of(attention_mask, B, H, Q, C, scores.device, 8)
    if mk is None:
        return None
    st = _stream_ptr(scores)
    fp8_out = _fp8_probs_times_v_or_none(st, scores, mk, scaling, fq_p, fq_v, value)
    if fp8_out is not None:
        return None, fp8_out                  # the probabilities exist only as FP8 codes on this path
    out = torch.empty_like(scores)
    fmt, lut, scale_ptr, amax_ptr = _probs_fq_launch_args(fq_p, scores.device, st, scores.numel())
    _native.check(_native.lib().qt_softmax_fq_bf16(scores.data_ptr(), mk.ptr, out.data_ptr(), B, H, Q, C, *mk.strides, float(scaling),
                                                   ctypes.byref(fmt), lut, scale_ptr, amax_ptr, st), "qt_softmax_fq_bf16")
    v = fq_v(value) if fq_v is not None else value
    return out, torch.matmul(out, v)


def _fp8_probs_times_v_or_none(st, scores, mk, scaling, fq_p, fq_v, value):
    """When the probabilities' and the values' fake-quantizers are stateless E4M3 / E5M2 ones, both tensors are exactly
    FP8: the score pass writes the probabilities' FP8 code only (1 B/element instead of 2), the value pass writes FP8
    next to bf16, and P.V runs as a batched FP8 GEMM (qt_fp8_gemm).  Same products, fp32 accumulation."""
    if (not switches.on("QT_FP8_ATTENTION") or not switches.on("QT_LT_GEMM") or not _LT["ok"]
            or fq_p is None or fq_v is None):
        return None
    if not (isinstance(fq_v, FusedAmaxObsFakeQuantize) and fq_p.producer_fusable() and fq_v.producer_fusable()):
        return None
    B, H, Q, C = scores.shape
    if value.dim() != 4 or value.shape[:3] != (B, H, C) or not readable_in_place(value):
        return None
    D = value.shape[-1]
    if D % 16 or C % 16 or B * H > 65535:
        return None
    if (B * H, Q, C, D) in _LT.setdefault("no_pv", set()):
        return None                            # the library had no kernel for this problem last time
    done = handover.done_by(value)
    v8 = handover.codes(value, unchecked=True)             # (unchecked read: used only beside the checked `done` below)
    if not (done is fq_v and v8 is not None and value.is_contiguous()):
        v8 = handover.fp8_view(fp8_codes_of_view(value, fq_v, st), fq_v)            # only the codes feed the FP8 P.V GEMM
    p8u = torch.empty((B, H, Q, C), dtype=torch.uint8, device=scores.device)
    # (qt_softmax_fq_bf16_fp8_live -- the same pass told each mask row's extent -- is bit-identical and gains a tenth alone on cold
    # buffers, nothing inside the window where the scores the Q.K^T GEMM just wrote are cache-resident: 12.97 against 12.88 ms; it
    # stays in the C ABI, the module path does not take it)
    _native.check(_native.lib().qt_softmax_fq_bf16_fp8(scores.data_ptr(), mk.ptr, None, p8u.data_ptr(), B, H, Q, C, *mk.strides, float(scaling),
                                                       ctypes.byref(fq_p._qt_format), st), "qt_softmax_fq_bf16_fp8")
    p8 = handover.fp8_view(p8u, fq_p)
    out = lt_fp8_gemm(p8.view(B * H, Q, C), v8.view(B * H, C, D), None, b_is_kn=True)
    if out is None:
        _LT["no_pv"].add((B * H, Q, C, D))     # the bf16 path redoes (and counts) the two passes
        return None
    STATS.add(value.numel())                   # the two fake-quant calls the reference issues here (av_matmul's inputs)
    STATS.add(scores.numel())
    return out.view(B, H, Q, D)


def attention_output_plan(attn):
    """What qt_attention_fp8's epilogue does for the consumer of its result: (fq_o, codes_only).  fq_o: the output projection's
    stateless FP8 input fake-quantizer when the kernel may apply it, else None.  codes_only (model_fusions.codes_only_ok): the projection
    multiplies the codes and nobody else can see the result -- no hook on the attention module but the package's own context hooks
    (which is why the module is not handed to codes_only_ok as the producer), none on the projection or its fake-quantizer -- so the
    kernel writes ONLY the codes and the bf16 tensor stays unwritten (`_qt_lazy`; whoever asks for the values
    after all gets them decoded: handover.materialize, through HF's reshaped view too)."""
    from .model_fusions import codes_only_ok, consumer_fq
    own = getattr(attn, "o_proj", None)
    proj = own or attn.__dict__.get("_qt_out_proj")                                 # LLaMA's own / BERT's BertSelfOutput.dense
    fq_o = consumer_fq(proj) if (proj is not None and switches.on("QT_FUSED_PRODUCER_FQ")) else None
    # (codes only where the projection is the block's own: the result then never leaves the attention module's forward.  BERT's
    # BertSelfAttention RETURNS it to its parent, which hands it to BertSelfOutput -- it keeps its values)
    return fq_o, fq_o is not None and own is not None and pc.no_foreign_hooks(attn) and codes_only_ok([proj])


def _attention_fp8_or_none(attn, query, key, value, attention_mask, scaling, fqs):
    """qt_attention_fp8: the attention core in one launch on FP8 codes (head_dim 128 or 64, keys in blocks of 128 up to 1024) when the
    four fake-quantizers around the two matmuls are stateless E4M3 / E5M2 ones of one format.  q / k either arrive with their codes (the
    rotary kernel attaches them) or are [B, H, S, D] views of the projections' outputs (BERT's transpose_for_scores), whose codes a
    codes-only pass over the view writes here -- that pass IS the fq_q / fq_k call.  Counts the four fake-quant calls the reference
    issues: q and k (handed through by their modules, or the passes just named), the value pass (qt_value_codes_t) and the
    probabilities inside the kernel.  Returns [B, Sq, H, D] or None."""
    fq_q, fq_k, fq_p, fq_v = fqs
    B, H, Q, D = query.shape
    C = key.shape[2]
    if D not in (64, 128) or C % 128 != 0 or C > 1024 or B * H > 65535:
        return None
    if not all(isinstance(f, FusedAmaxObsFakeQuantize) and f.producer_fusable() for f in fqs):
        return None
    if len({f._qt_format.key() for f in fqs}) != 1 or not readable_in_place(value):
        return None

    def handed(t, fq, rows):
        t8 = handover.codes(t)
        if t8 is None or handover.done_by(t) is not fq or not t8.is_contiguous() or tuple(t8.shape) != (B, H, rows, D):
            return None
        return t8

    q8, k8 = handed(query, fq_q, Q), handed(key, fq_k, C)
    if (q8 is None and not readable_in_place(query)) or (k8 is None and not readable_in_place(key)):
        return None
    mk = AttentionMask.of(attention_mask, B, H, Q, C, query.device, 4)
    if mk is None:
        return None
    L = _native.lib()
    st = _stream_ptr(query)
    live = mk.row_live(B, H, Q, C, st)

    def codes(t, fq, t8):
        if t8 is not None:
            # hand-over, counted as the fake-quantizer's own forward would (calling it would also decode codes-only tensors, see
            # model_fusions.rope_fq: nothing here reads the bf16 values)
            count_call(fq, t.numel())
            return t8
        t8 = fp8_codes_of_view(t, fq, st)
        STATS.add(t.numel())
        return t8

    def token_rows(t):
        """Row stride when `t` is the [B, H, S, D] view of a [B, S, H, D]-ordered buffer (transpose_for_scores of a projection), else None."""
        b_, h_, s_, d_ = t.shape
        rs = t.stride(2)
        return rs if (t.stride(3) == 1 and t.stride(1) == d_ and t.stride(0) == s_ * rs and rs % 8 == 0 and rs >= h_ * d_) else None

    vt8 = None
    if (q8 is None and k8 is None and Q == C and key.shape[1] == H and value.shape[1] == H and token_rows(query) is not None
            and token_rows(key) is not None and switches.on("QT_ROPE_VALUE_LAUNCH")):
        # q and k codes and the value codes in ONE launch (qt_rope_fq_value without a rotation): the three calls fq_q, fq_k, fq_v
        q8 = torch.empty((B, H, Q, D), dtype=torch.uint8, device=query.device)
        k8 = torch.empty((B, H, C, D), dtype=torch.uint8, device=query.device)
        vt8 = torch.empty((B, H, D, C), dtype=torch.uint8, device=query.device)
        _native.check(L.qt_rope_fq_value(query.data_ptr(), key.data_ptr(), None, None, None, None, q8.data_ptr(), k8.data_ptr(), B, Q, H, H, D,
                                         token_rows(query), token_rows(key), ctypes.byref(fq_q._qt_format), ctypes.byref(fq_k._qt_format),
                                         value.data_ptr(), vt8.data_ptr(), value.stride(0), value.stride(1), value.stride(2),
                                         ctypes.byref(fq_v._qt_format), st), "qt_rope_fq_value")
        STATS.add(query.numel())
        STATS.add(key.numel())
    else:
        q8, k8 = codes(query, fq_q, q8), codes(key, fq_k, k8)
    fmt = fq_v._qt_format
    early = precomputed.VALUE_CODES_T.take(attn, value)
    if vt8 is not None:
        pass                                                 # written by the launch above
    elif isinstance(early, tuple) and early[0] is fq_v:
        vt8 = early[1]                                       # written by the launch that carried the rotary kernel (model_fusions.rope_fq)
    else:
        vt8 = torch.empty((B, H, D, C), dtype=torch.uint8, device=query.device)
        _native.check(L.qt_value_codes_t(value.data_ptr(), vt8.data_ptr(), B, H, C, D, value.stride(0), value.stride(1), value.stride(2),
                                         ctypes.byref(fmt), st), "qt_value_codes_t")
    STATS.add(value.numel())                                 # fq_v, evaluated by that pass
    STATS.add(B * H * Q * C)                                 # fq_p, evaluated inside the kernel
    # the output projection's stateless FP8 input fake-quantizer rides on the epilogue (as model_fusions.attention_output does for the
    # library-GEMM chain): HF reshapes the result before the projection's hook sees it, so the hand-over is an expectation
    fq_o, codes_only = attention_output_plan(attn)
    out8 = torch.empty((B, Q, H, D), dtype=torch.uint8, device=query.device) if fq_o is not None else None
    shape = (B, Q, H, D)
    out = handover.unwritten(shape, torch.bfloat16, query.device) if codes_only else torch.empty(shape, dtype=torch.bfloat16, device=query.device)
    _native.check(L.qt_attention_fp8(q8.data_ptr(), k8.data_ptr(), vt8.data_ptr(), 1 if fmt.p0 == 2 else 0, mk.ptr, *mk.strides, *live[:4], 0, live[4],
                                     None if codes_only else out.data_ptr(), out8.data_ptr() if out8 is not None else None,
                                     ctypes.byref(fq_o._qt_format) if fq_o is not None else None, B, H, Q, C, D, float(scaling), st),
                  "qt_attention_fp8")
    if codes_only:
        handover.stamp(out, fq_o, handover.fp8_view(out8, fq_o), lazy=True)
    if fq_o is not None:
        fq_o.expect_prequantized(out, handover.fp8_view(out8, fq_o))
    return out


def fused_attention_or_none(attn, query, key, value, attention_mask, scaling, dropout):
    """The whole attention core in ONE HIP launch (qt_attention_fq_bf16): QK^T, scaling, mask, softmax,
    fake-quant of the probabilities and P.V on the matrix cores, the S x S tensor never written.  q, k, v go
    through their own per-tensor fake-quantizers first (elementwise passes that also write the contiguous
    [B, H, S, D] layout).  Same applicability rules as the fused score path, plus head_dim in {64, 128};
    returns the attention output already in [B, Sq, H, D], or None.

    QT_FUSED_ATTENTION: "0" never, "1" whenever applicable, unset = only head_dim 64, where the kernel measured
    faster than the library-GEMM chain (B16 H12 S384: 85 vs 113 us); at head_dim 128 the chain wins (92 vs 122 us at
    B1 H32 S1024), so the chain stays the default there."""
    mode = switches.mode("QT_FUSED_ATTENTION")
    fp8_kernel = query.dim() == 4 and query.shape[-1] in (64, 128) and switches.on("QT_FP8_ATTENTION_KERNEL")
    if mode == "0" or (mode != "1" and query.shape[-1] != 64 and not fp8_kernel):
        return None
    if not (query.device.type == "cuda" and query.dtype == torch.bfloat16 and query.dim() == 4):
        return None
    if torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad):
        return None
    if dropout and attn.training:
        return None
    B, H, Q, D = query.shape
    C = key.shape[2]
    if D not in (64, 128) or C % 4 != 0 or key.shape != (B, H, C, D) or value.shape != (B, H, C, D) or B * H > 65535:
        return None
    # (backward hooks are looked at on none of the four modules: this is the no_grad path -- gradients were declined above)
    for mod in (attn.attn_scaling, attn.softmax):
        if getattr(mod, "activation_pre_process", None) is not None or not pc.no_forward_hooks(mod):
            return None
    hq, hv = getattr(attn.qk_matmul, "activation_pre_process", None), getattr(attn.av_matmul, "activation_pre_process", None)
    if (hq is None) != (hv is None):
        return None
    fq_q = fq_k = fq_p = fq_v = None
    # quantize()'s one pre-hook per matmul with its holder, no hook at all without; never a forward hook
    if not all(pc.quantize_hooks_only(mod, 0 if hq is None else 1) for mod in (attn.qk_matmul, attn.av_matmul)):
        return None
    if hq is not None:
        fqs_qk, fqs_av = (pc.holder_fqs(mod, "activation_pre_process", "0", "1", exact=False) for mod in (attn.qk_matmul, attn.av_matmul))
        if fqs_qk is None or fqs_av is None:
            return None                       # first call: let the hooks create the fake-quantizers
        fq_q, fq_k, fq_p, fq_v = *fqs_qk, *fqs_av
        if not all(pc.plain_per_tensor(f) for f in (fq_q, fq_k, fq_p, fq_v)):
            return None
    if fp8_kernel and fq_q is not None and switches.on("QT_FP8_ATTENTION"):
        out = _attention_fp8_or_none(attn, query, key, value, attention_mask, scaling, (fq_q, fq_k, fq_p, fq_v))
        if out is not None:
            return out
    table_p = (fq_p is not None and fq_p._quantize and fq_p._qt_format.kind == _native.QT_FMT_LUT)
    if mode != "1" and query.shape[-1] != 64 and not table_p:
        # head_dim 128 without the FP8 kernel: the library-GEMM chain (see above) -- except for table formats (posit, fpN, ...),
        # whose chain pays an LDS-table softmax pass and three strided fake-quant passes: LLaMA-2-13B posit8_2 window 42.6 -> 40.6 ms
        return None
    mk = AttentionMask.of(attention_mask, B, H, Q, C, query.device, 4)
    if mk is None:
        return None
    st = _stream_ptr(query)
    qq = (fq_q(query) if fq_q is not None else query).contiguous()
    kq = (fq_k(key) if fq_k is not None else key).contiguous()          # K, not K^T: elementwise, same statistics
    fmt, lut, scale_ptr, amax_ptr = _probs_fq_launch_args(fq_p, query.device, st, B * H * Q * C, drop_unit_scale=True)
    stateless_table = table_p and scale_ptr is None and amax_ptr is None
    # table formats: the output projection's stateless input fake-quantizer of the SAME format rides on the kernel's epilogue (its hook
    # then hands the result through: fake_quantize.expect_prequantized)
    fq_o = None
    if stateless_table and (fmt.p1 & 1) and switches.on("QT_FUSED_PRODUCER_FQ") and switches.on("QT_FUSED_PRODUCER_MAP"):
        from .model_fusions import consumer_fq_map
        proj = getattr(attn, "o_proj", None) or attn.__dict__.get("_qt_out_proj")
        cand = consumer_fq_map(proj) if proj is not None else None
        if cand is not None and cand.dtype == fq_p.dtype:
            fq_o = cand
    return table_format_core(attn, st, qq, kq, value, fq_v, mk, (B, H, Q, C, D), scaling, fmt, lut, fq_o, scale_ptr, amax_ptr,
                             rows=stateless_table and fq_v is not None and pc.no_forward_hooks(fq_v))


def table_format_core(attn, st, qq, kq, value, fq_v, mk, dims, scaling, fmt, lut, fq_o, scale_ptr=None, amax_ptr=None, rows=True):
    """The core on bf16 matrix instructions from fake-quantized contiguous q / k and the UNQUANTIZED `value`, [B, Sq, H, D]:
    qt_attention_rows_bf16 where `rows` allows and it takes the problem, else fq_v's own pass + the two-pass kernel; then the expectation
    for the output projection's input fake-quantizer `fq_o` (None: nobody's), which the kernel applied in its epilogue."""
    B, H, Q, C, D = dims
    out = torch.empty((B, Q, H, D), dtype=torch.bfloat16, device=qq.device)
    if not (rows and attention_rows_or_none(attn, st, qq, kq, value, fq_v, mk, out, dims, scaling, fmt, lut, fq_o is not None)):
        vq = (fq_v(value) if fq_v is not None else value).contiguous()
        launch_attention_fq(st, qq, kq, vq, mk, out, dims, scaling, fmt, lut, scale_ptr, amax_ptr, fq_o is not None)
    if fq_o is not None:
        fq_o.expect_prequantized(out, None)
    return out


def attention_rows_or_none(attn, st, qq, kq, value, fq_v, mk, out, dims, scaling, fmt, lut, out_fq):
    """qt_attention_rows_bf16 (round 4): the table-format attention core with the score strip in registers -- head_dim 128, key counts in
    blocks of 128 up to 1024, the probabilities' fake-quantizer a stateless table format in its row form (fmt / lut as handed to
    launch_attention_fq), and `fq_v` a stateless table format in its row form too: its call IS the kernel's value pass
    (qt_value_t_rows: fq_v(value), transposed, keys in the k-slot order), counted here.  `value`: the UNQUANTIZED [B, H, C, D] view.
    Returns True when the launch was made; False: the caller takes the two-pass kernel."""
    B, H, Q, C, D = dims
    if D != 128 or C % 128 != 0 or C > 1024 or B * H > 65535 or not (fmt.kind == _native.QT_FMT_LUT and (fmt.p1 & 1)) or lut is None:
        return False
    if not (isinstance(fq_v, FusedAmaxObsFakeQuantize) and fq_v.stateless_map() and fq_v._qt_format.kind == _native.QT_FMT_LUT):
        return False
    fq_v._move_to(value.device)
    vfmt = _launch_format(fq_v._qt_format, fq_v.qmap)
    if not (vfmt.p1 & 1) or not readable_in_place(value):
        return False
    # everything qt_attention_rows_bf16 would refuse, BEFORE the value pass is issued and counted
    if (qq.data_ptr() | kq.data_ptr() | lut) % 16 or out.data_ptr() % 8:
        return False
    if mk.view is not None and (mk.ptr % 8 or (mk.strides[0] | mk.strides[1] | mk.strides[2]) % 4):
        return False
    L = _native.lib()
    live = mk.row_live(B, H, Q, C, st)
    early = precomputed.VALUE_T_ROWS.take(attn, value)
    if isinstance(early, tuple) and early[0] is fq_v:
        vt = early[1]                                          # written by the launch that carried the rotary kernel (model_fusions.rope_map)
    else:
        vt = torch.empty((B, H, D, C), dtype=torch.bfloat16, device=value.device)
        _native.check(L.qt_value_t_rows(value.data_ptr(), vt.data_ptr(), B, H, C, D, value.stride(0), value.stride(1), value.stride(2),
                                        ctypes.byref(vfmt), fq_v.qmap.data_ptr(), st), "qt_value_t_rows")
    count_call(fq_v, value.numel())                            # the fq_v call
    _native.check(L.qt_attention_rows_bf16(qq.data_ptr(), kq.data_ptr(), vt.data_ptr(), mk.ptr, *mk.strides, *live, out.data_ptr(), int(bool(out_fq)),
                                           ctypes.byref(fmt), lut, B, H, Q, C, D, float(scaling), st), "qt_attention_rows_bf16")
    return True


def launch_attention_fq(st, qq, kq, vq, mk, out, dims, scaling, fmt, lut, scale_ptr, amax_ptr, out_fq):
    """qt_attention_fq_bf16 / _out_ / _live_: with a mask whose rows are evenly spaced the launch carries the mask's row extents
    (AttentionMask.row_live: scanned once per mask object), and the kernel does not read a causal / right-padding mask at all."""
    B, H, Q, C, D = dims
    L = _native.lib()
    live = mk.row_live(B, H, Q, C, st)
    if live[0] is not None:
        _native.check(L.qt_attention_fq_live_bf16(qq.data_ptr(), kq.data_ptr(), vq.data_ptr(), mk.ptr, out.data_ptr(), B, H, Q, C, D, *mk.strides,
                                                  float(scaling), ctypes.byref(fmt), lut, scale_ptr, amax_ptr, int(bool(out_fq)), *live, st),
                      "qt_attention_fq_live_bf16")
    elif out_fq:
        _native.check(L.qt_attention_fq_out_bf16(qq.data_ptr(), kq.data_ptr(), vq.data_ptr(), mk.ptr, out.data_ptr(), B, H, Q, C, D, *mk.strides,
                                                 float(scaling), ctypes.byref(fmt), lut, st), "qt_attention_fq_out_bf16")
    else:
        _native.check(L.qt_attention_fq_bf16(qq.data_ptr(), kq.data_ptr(), vq.data_ptr(), mk.ptr, out.data_ptr(), B, H, Q, C, D, *mk.strides,
                                             float(scaling), ctypes.byref(fmt), lut, scale_ptr, amax_ptr, st), "qt_attention_fq_bf16")
