"""CPU ORACLE -- TEST INFRASTRUCTURE ONLY.

A numpy restatement of the reference's fake-quantization hot path.  It exists so
that the HIP kernels can be checked against an independent statement of the
algorithm on hosts where the reference itself is absent (the GPU box).

  * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
    import this package.  The product (quantized-training_amd/) never does; it
    raises if its HIP library is missing.
  * Parity is PINNED: every function below is checked against golden vectors
    produced by running the reference in the build container
    (tests/golden/gen_golden.py -> tests/golden/*.npz, tests/test_oracle_golden.py).

All file:line citations are relative to the upstream checkout
(src/quantized_training/...).  Values travel as bit patterns: bf16 tensors are
uint16 arrays, fp32 tensors are float32 arrays (or their uint32 view).
"""
import math
import re
from typing import NamedTuple, Optional

import numpy as np

U16 = np.uint16
U32 = np.uint32
F32 = np.float32


# --------------------------------------------------------------------------
# bf16 helpers (value <-> bit pattern); torch semantics: RNE, NaN stays NaN
# --------------------------------------------------------------------------
def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=U16).astype(U32) << U32(16)).view(F32)


def f32_to_bf16(x):
    """float32 -> bf16 bits, round-to-nearest-even, NaN -> quiet NaN (0x7FC0)."""
    x = np.ascontiguousarray(x, dtype=F32)
    b = x.view(U32)
    r = ((b + U32(0x7FFF) + ((b >> U32(16)) & U32(1))) >> U32(16)).astype(U16)
    return np.where(np.isnan(x), U16(0x7FC0), r).astype(U16)


def rbf(x):
    """Round a float32 array to the nearest bf16-representable float32."""
    return bf16_to_f32(f32_to_bf16(x))


def all_bf16_patterns():
    return np.arange(65536, dtype=U32).astype(U16)


def canon_nan16(bits):
    bits = np.array(bits, dtype=U16, copy=True)
    nan = ((bits & 0x7F80) == 0x7F80) & ((bits & 0x007F) != 0)
    bits[nan] = 0x7FC0
    return bits


def canon_nan32(bits):
    bits = np.array(bits, dtype=U32, copy=True)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)
    bits[nan] = 0x7FC00000
    return bits


# --------------------------------------------------------------------------
# A2: NVIDIA-style FP8 rounding on the fp32 image (fp8.py:10-67)
# --------------------------------------------------------------------------
def quantize_to_fp8(x, mbits, fp8_max, fp8_min):
    """fp8.py:10-37 (e4m3: mbits=3, max 448, min 2^-6) / :40-67 (e5m2: 2, 57344, 2^-14).
    x: float32 array; returns float32 array."""
    x = np.ascontiguousarray(x, dtype=F32)
    raw = x.view(U32).astype(np.int64)
    sign = raw & 0x80000000
    exp = ((raw & 0x7F800000) >> 23) - 127                      # :17
    frac = (raw & 0x7FFFFF) | 0x800000                           # :18
    min_exp = int(math.floor(math.log2(fp8_min)))                # :20
    nf = 23 - mbits + np.clip(min_exp - exp, 0, None)            # :21
    nfs = np.minimum(nf, 40)                                     # int64 shifts stay defined; tiny inputs are flushed below
    lb = (frac & (1 << nfs)) != 0                                # :22
    gb = (frac & (1 << (nfs - 1))) != 0                          # :23
    sb = (frac & ((1 << (nfs - 1)) - 1)) != 0                    # :24
    rb = (lb & gb) | (gb & sb)                                   # :25
    nfc = np.minimum(nf, 23)                                     # :27
    mag = (raw & 0x7FFFFFFF) & ~((1 << nfc) - 1)                 # :28
    mag = np.where(rb, mag + (1 << nfc), mag)                    # :29
    out = (mag | sign).astype(U32).view(F32)
    with np.errstate(invalid="ignore"):
        out = np.clip(out, -F32(fp8_max), F32(fp8_max))          # :32
        out = np.where(np.abs(x) <= F32(fp8_min * 2.0 ** -(mbits + 1)), F32(0), out)   # :33
        out = np.where(x == 0, F32(0), out)                      # :35
    out = np.where(np.isfinite(x), out, F32(np.nan))             # :36
    return out.astype(F32)


def quantize_to_fp8_e4m3(x):
    return quantize_to_fp8(x, 3, 448.0, 2.0 ** -6)


def quantize_to_fp8_e5m2(x):
    return quantize_to_fp8(x, 2, 57344.0, 2.0 ** -14)


# --------------------------------------------------------------------------
# A4: posit<nbits,es> rounding (posit.py:6-67)
# --------------------------------------------------------------------------
def quantize_to_posit(x, nbits, es):
    """posit.py:6-67 with round_to_even=True.  x: float32 array -> float32 array."""
    x = np.ascontiguousarray(x, dtype=F32)
    raw = x.view(U32).astype(np.int64)
    scale = ((raw & 0x7F800000) >> 23) - 127                     # :14
    frac = raw & 0x7FFFFF                                        # :15
    r = scale >= 0                                               # :16
    max_scale = (nbits - 2) * (1 << es)                          # :18
    dominated = np.where(r, scale > max_scale, scale < -max_scale)   # :19
    run = np.where(r, 1 + (scale >> es), -(scale >> es))         # :21 (arithmetic shift == floor)
    run_s = np.minimum(run, 30)                                  # keep shifts defined; dominated lanes ignore rb
    regime = np.where(r, (1 << (run_s + 1)) - 1, 0) ^ 1          # :22
    exponent = scale % (1 << es)                                 # :23 (floor-mod)
    pt = (regime << (23 + es)) | (exponent << 23) | frac         # :24
    ln = 2 + run_s + es + 23                                     # :27
    sh = np.clip(ln - nbits, 1, 62)
    lbm = 1 << sh                                                # :28
    gbm = lbm >> 1                                               # :29
    sbm = gbm - 1                                                # :30
    lb = (pt & lbm) != 0
    gb = (pt & gbm) != 0
    sb = (pt & sbm) != 0
    rb = ((lb & gb) | (gb & sb)) & ~dominated                    # :35
    ne = np.clip(2 + run + es - nbits, 0, es)                    # :38
    sc = scale & ~((1 << ne) - 1)                                # :39 (two's complement and)
    sc = np.clip(sc, -max_scale, max_scale)                      # :40
    nf = np.clip(2 + run + es + 23 - nbits, 0, 23)               # :43
    fr = frac & ~((1 << nf) - 1)                                 # :44
    out = ((sc + 127) << 23) | fr                                # :46
    out = np.where(rb, out + (1 << (nf + ne)), out)              # :47
    with np.errstate(invalid="ignore", over="ignore"):
        mag = (out & 0xFFFFFFFF).astype(U32).view(F32)
        out = mag * np.sign(x)                                   # :48
        thr = math.pow(2, math.floor(-(nbits - 1) * (1 << es) + 2 ** (es - 1)))   # :52
        out = np.where(np.abs(x) < F32(thr), F32(0), out)        # :53
        out = np.where(x == 0, F32(0), out)                      # :56
    out = np.where(np.isfinite(x), out, F32(np.nan))             # :57
    return out.astype(F32)


# --------------------------------------------------------------------------
# A3: MX-library float rounding evaluated in bf16 arithmetic (fp8.py:147-203
#     called on a bf16 tensor from fake_quantize.py:63-80)
# --------------------------------------------------------------------------
def _clamp(a, lo, hi):
    """torch.clamp: min(max(a, lo), hi) with std::max/min operand order (keeps -0.0, NaN)."""
    with np.errstate(invalid="ignore"):
        a = np.where(a < lo, lo, a)
        a = np.where(a > hi, hi, a)
    return a


def _sign(a):
    with np.errstate(invalid="ignore"):
        s = (a > 0).astype(F32) - (a < 0).astype(F32)
    return np.where(np.isnan(a), F32(np.nan), s).astype(F32)


def quantize_elemwise_core_bf16(bits_in, bits, exp_bits, max_norm):
    """_quantize_elemwise_core(A:bf16, bits, exp_bits, max_norm, round='even',
    saturate_normals=True) -- fp8.py:147-203; every torch op rounds to bf16."""
    A = bf16_to_f32(bits_in)
    with np.errstate(all="ignore"):
        absA = np.abs(A)
        t = rbf(absA + (A == 0).astype(F32))                       # :174-175
        pe = np.floor(rbf(np.log2(t).astype(F32)))                 # :174
        min_exp = -(2 ** (exp_bits - 1)) + 2                       # :178
        pe = np.where(pe < min_exp, F32(min_exp), pe).astype(F32)  # :179 (NaN stays NaN)
        p2 = rbf(np.exp2(pe.astype(np.float64)).astype(F32))       # 2 ** private_exp  (:94)
        out = rbf(rbf(A / p2) * F32(2 ** (bits - 2)))              # _safe_lshift :90-94
        # _round_mantissa(..., 'even')  :123-127
        a = np.abs(out)
        am = rbf(a - F32(0.5))
        rem = am - F32(2) * np.floor(am / F32(2))                  # python-style remainder, exact
        mask = (rem == 0).astype(F32)
        mask = np.where(np.isnan(am), F32(0), mask)
        fl = rbf(np.floor(rbf(a + F32(0.5))) - mask)
        out = rbf(_sign(out) * fl)
        out = rbf(rbf(out / F32(2 ** (bits - 2))) * p2)            # _safe_rshift :97-101
        out = _clamp(out, -rbf(np.array(max_norm, F32)), rbf(np.array(max_norm, F32)))   # :193
        out = np.where(A == np.inf, F32(np.inf), out)              # :199
        out = np.where(A == -np.inf, F32(-np.inf), out)            # :200
    return f32_to_bf16(out.astype(F32))


# --------------------------------------------------------------------------
# A1: the 65 536-entry value map (fake_quantize.py:31-95)
# --------------------------------------------------------------------------
def get_quantization_map(dtype):
    """Returns uint16[65536]: bf16 bits of Q_dtype(bf16_from_bits(i)).  NaNs canonical (0x7FC0)."""
    idx = all_bf16_patterns()
    vals = bf16_to_f32(idx)
    if dtype is None:                                              # :34-35
        return canon_nan16(idx)
    if dtype in ("float32", "bfloat16"):                           # :38-40
        return canon_nan16(idx)
    if dtype == "float16":
        with np.errstate(over="ignore", invalid="ignore"):
            return canon_nan16(f32_to_bf16(vals.astype(np.float16).astype(F32)))
    m = re.fullmatch(r"int(\d+)", dtype, re.IGNORECASE)            # :43-46
    u = re.fullmatch(r"uint(\d+)", dtype, re.IGNORECASE)           # :49-52
    if m or u:
        n = int((m or u).group(1))
        lo, hi = (-(2 ** (n - 1)), 2 ** (n - 1) - 1) if m else (0, 2 ** n - 1)
        lo = rbf(np.array(lo, F32))                                # clamp bounds are cast to the tensor dtype
        hi = rbf(np.array(hi, F32))
        with np.errstate(invalid="ignore"):
            r = np.rint(vals)                                      # round-half-even, exact in bf16
        return canon_nan16(f32_to_bf16(_clamp(r, lo, hi)))
    m = re.fullmatch(r"(?:fp8\.)?(e4m3|e5m2)", dtype, re.IGNORECASE)   # :55-60
    if m:
        f = quantize_to_fp8_e4m3 if m.group(1).lower() == "e4m3" else quantize_to_fp8_e5m2
        return canon_nan16(f32_to_bf16(f(vals)))
    m = re.fullmatch(r"fp(\d+)_e(\d+)m(\d+)", dtype)               # :63-80
    if m:
        nbits, ebits, mbits = map(int, m.groups())
        assert nbits == ebits + mbits + 1 or nbits == ebits + mbits
        src = idx
        if nbits == ebits + mbits:                                 # unsigned: abs first (:68-69)
            src = idx & U16(0x7FFF)
        mb = mbits + 2
        emax = 2 ** (ebits - 1) - 1 if ebits > 4 else 2 ** (ebits - 1)
        if dtype != "fp8_e4m3":
            max_norm = 2 ** emax * float(2 ** (mb - 1) - 1) / 2 ** (mb - 2)
        else:
            max_norm = 2 ** emax * 1.75
        return canon_nan16(quantize_elemwise_core_bf16(src, mb, ebits, max_norm))
    m = re.fullmatch(r"posit(\d+)_(\d+)", dtype)                   # :84-86
    if m:
        return canon_nan16(f32_to_bf16(quantize_to_posit(vals, int(m.group(1)), int(m.group(2)))))
    m = re.fullmatch(r"nf(\d+)(?:_(\d+))?", dtype)                # :90-93 (flattened: values[indices])
    if m:
        return canon_nan16(nf_value_map(int(m.group(1)), int(m.group(2)) if m.group(2) else None))
    raise ValueError(f"Unsupported dtype: {dtype}")                # :95


# --------------------------------------------------------------------------
# NormalFloat code books (normal_float.py:4-62): 2^k levels at evenly spaced N(0,1) quantiles
# --------------------------------------------------------------------------
def nf_levels(k=4, int_bits=None, offset=0.9677083):
    from scipy.stats import norm
    half = 2 ** (k - 1)

    def lin(steps):          # torch.linspace(offset, 0.5, steps) in float32 (two-sided evaluation)
        step = (F32(0.5) - F32(offset)) / F32(steps - 1)
        i = np.arange(steps, dtype=F32)
        return np.where(np.arange(steps) < steps // 2, F32(offset) + step * i,
                        F32(0.5) - step * (F32(steps - 1) - i)).astype(F32)

    v = np.concatenate([norm.ppf(lin(half + 1)[:-1]), [0.0], -norm.ppf(lin(half)[:-1])]).astype(F32)   # :13-16
    v = np.sort(v)
    v = (v / v.max()).astype(F32)                                                                        # :26-27
    if int_bits is not None:
        v = np.rint(v * F32(2 ** (int_bits - 1) - 1)).astype(F32)                                        # :52-54
    return v


def nf_value_map(k=4, int_bits=None):
    """bf16 bits of values[argmin |values - clamp(x)|] for every bf16 pattern (normal_float.py:56-60)."""
    levels = rbf(nf_levels(k, int_bits))                                                                 # values.to(bf16)
    x = bf16_to_f32(all_bf16_patterns())
    with np.errstate(invalid="ignore"):
        xc = _clamp(x, levels.min(), levels.max())
        dist = np.abs(rbf(levels[None, :] - xc[:, None]))                                                # bf16 subtraction
        dist = np.where(np.isnan(dist), F32(np.inf), dist)
        nanrow = np.isnan(xc)
        idx = np.argmin(dist, axis=1)
    out = f32_to_bf16(levels[idx])
    # torch.argmin on an all-NaN row returns the first NaN position (index 0)
    out[nanrow] = f32_to_bf16(levels[:1])[0]
    return out


# --------------------------------------------------------------------------
# A5: vmap (decomposed.py:146-163)
# --------------------------------------------------------------------------
def vmap_index_f32(x):
    """decomposed.py:151-153: hi16(bits) | (lo16 != 0)"""
    b = np.ascontiguousarray(x, dtype=F32).view(U32)
    return ((b >> U32(16)) | ((b & U32(0xFFFF)) != 0).astype(U32)).astype(U16)


def vmap_bf16(xbits, qmap):
    """bf16 tensor (uint16 bits) -> bf16 bits (decomposed.py:148-149,159-161)."""
    return np.asarray(qmap, dtype=U16)[np.asarray(xbits, dtype=U16)]


def vmap_f32(x, qmap):
    """float32 tensor -> float32 tensor (qmap value cast to the output dtype)."""
    return bf16_to_f32(np.asarray(qmap, dtype=U16)[vmap_index_f32(x)])


def vmap_f16(xbits_f16, qmap):
    """float16 bits -> float16 bits: index through the fp32 image, value cast bf16->fp16."""
    x = np.asarray(xbits_f16, dtype=U16).view(np.float16).astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return vmap_f32(x, qmap).astype(np.float16).view(U16)


# --------------------------------------------------------------------------
# A6/A7: quantize / dequantize / fake-quant with a scale, in the input dtype
# --------------------------------------------------------------------------
def fq_bf16(xbits, qmap, scale_bits):
    """y = vmap(x / s, qmap) * s on bf16 tensors; s is bf16 (bits), broadcastable.
    fake_quantize.py:245-246: each op computed in fp32 and rounded to bf16."""
    x = bf16_to_f32(xbits)
    s = bf16_to_f32(scale_bits)
    with np.errstate(all="ignore"):
        q = vmap_bf16(f32_to_bf16((x / s).astype(F32)), qmap)
        return f32_to_bf16((bf16_to_f32(q) * s).astype(F32))


def fq_f32(x, qmap, scale):
    x = np.ascontiguousarray(x, dtype=F32)
    s = np.asarray(scale, dtype=F32)
    with np.errstate(all="ignore"):
        return (vmap_f32((x / s).astype(F32), qmap) * s).astype(F32)


def quantize_f32(x, qmap, scale, zero_point=None):
    """decomposed.py:205-210"""
    with np.errstate(all="ignore"):
        t = (np.asarray(x, F32) / np.asarray(scale, F32)).astype(F32)
        if zero_point is not None:
            t = (t + np.asarray(zero_point, F32)).astype(F32)
    return vmap_f32(t, qmap)


def quantize_bf16(xbits, qmap, scale_bits):
    with np.errstate(all="ignore"):
        t = f32_to_bf16((bf16_to_f32(xbits) / bf16_to_f32(scale_bits)).astype(F32))
    return vmap_bf16(t, qmap)


def dequantize_f32(x, scale, zero_point=None, input_qmap=None, output_qmap=None):
    """decomposed.py:246-262"""
    x = np.asarray(x, F32)
    if input_qmap is not None:
        x = vmap_f32(x, input_qmap)
    with np.errstate(all="ignore"):
        if zero_point is not None:
            x = (x - np.asarray(zero_point, F32)).astype(F32)
        y = (x * np.asarray(scale, F32)).astype(F32)
    if output_qmap is not None:
        y = vmap_f32(y, output_qmap)
    return y


def dequantize_bf16(xbits, scale_bits, input_qmap=None, output_qmap=None):
    if input_qmap is not None:
        xbits = vmap_bf16(xbits, input_qmap)
    with np.errstate(all="ignore"):
        y = f32_to_bf16((bf16_to_f32(xbits) * bf16_to_f32(scale_bits)).astype(F32))
    if output_qmap is not None:
        y = vmap_bf16(y, output_qmap)
    return y


class FakeQuantState:
    """The buffers FusedAmaxObsFakeQuantFunction mutates (fake_quantize.py:304-312)."""

    def __init__(self, amax_history_len, quant_max, observer=True, ch_axis=None, per_channel=False, pow2=False):
        self.amax_history = np.zeros((0,), F32)
        self.scale = np.ones((1,), F32)
        self.L = amax_history_len
        self.quant_max = quant_max
        self.observer_enabled = observer
        self.fake_quant_enabled = True
        self.ch_axis = ch_axis
        self.per_channel = per_channel
        self.pow2 = pow2


def _amax_f32(x, st):
    """fake_quantize.py:218-223; NaN propagates like torch.amax."""
    a = np.abs(x)
    if st.per_channel:
        ax = st.ch_axis + x.ndim if st.ch_axis < 0 else st.ch_axis
        dims = tuple(i for i in range(x.ndim) if i != ax)
        return np.max(a, axis=dims, keepdims=True).astype(F32)       # np.max propagates NaN
    return np.max(a).astype(F32).reshape(())


def fake_quant_forward(x, is_bf16, qmap, st):
    """fake_quantize.py:217-248.  x: float32 array holding the tensor VALUES (for bf16 tensors the
    values are bf16-representable).  Returns values as float32 (bf16-representable when is_bf16)."""
    x = np.ascontiguousarray(x, dtype=F32)
    if st.observer_enabled:
        amax_cur = _amax_f32(x, st)                                    # :218-223 (exact in either dtype)
        if st.amax_history.size == 0:                                  # :225-228
            st.amax_history = np.zeros((st.L,) + amax_cur.shape, F32)
            st.scale = np.ones(amax_cur.shape, F32)
        amax = np.max(st.amax_history, axis=0)                         # :230
        if st.amax_history.shape[0] > 1:                               # :232-234
            st.amax_history = np.roll(st.amax_history, -1, axis=0)
        st.amax_history[0] = amax_cur                                  # :235
        with np.errstate(all="ignore"):
            sf = (amax / F32(st.quant_max)).astype(F32)                # :237
            sf = np.where(amax > 0.0, sf, st.scale)                    # :238
            sf = np.where(np.isfinite(amax), sf, st.scale)             # :239
            if st.pow2:                                                # :240-241
                sf = np.exp2(np.ceil(np.log2(sf.astype(F32)))).astype(F32)
        st.scale = sf.astype(F32)                                      # :242
    if not st.fake_quant_enabled:
        return x
    if is_bf16:                                                        # :245-246
        sb = f32_to_bf16(st.scale)
        return bf16_to_f32(fq_bf16(f32_to_bf16(x), qmap, np.broadcast_to(sb, x.shape) if sb.ndim == x.ndim else sb))
    return fq_f32(x, qmap, st.scale)


# --------------------------------------------------------------------------
# H1: WikiText sliding-window schedule (examples/language_modeling/wikitext.py:143-165)
# --------------------------------------------------------------------------
def wikitext_windows(seq_len, max_length, stride):
    rows, prev_end = [], 0
    for begin in range(0, seq_len - max_length, stride):
        end = min(begin + max_length, seq_len)
        rows.append((begin, end, end - prev_end))
        prev_end = end
        if end == seq_len:
            break
    return rows


# --------------------------------------------------------------------------
# Block-scaled formats: microscaling and group-wise affine fake-quant
#   MXFakeQuantFunction            fake_quantize.py:98-133
#   calculate_mx_qparam/quantize_mx decomposed.py:365-448,  _reshape_to_blocks mx_utils.py:58-118
#   GroupWiseAffineFakeQuantFunction fake_quantize.py:136-194
# Every torch op on a bf16 tensor rounds its result to bf16; `rd` applies that rounding.
# --------------------------------------------------------------------------
def _to_blocks(x, axis, bs):
    """[..., n, ...] -> [..., nblk, bs, ...] zero-padded along `axis` (mx_utils.py:58-118)."""
    ax = axis % x.ndim
    n = x.shape[ax]
    pad = (-n) % bs
    if pad:
        w = [(0, 0)] * x.ndim
        w[ax] = (0, pad)
        x = np.pad(x, w)
    shp = list(x.shape)
    shp[ax:ax + 1] = [x.shape[ax] // bs, bs]
    return x.reshape(shp), ax


def _expand_blocks(s, ax, bs, n):
    return np.repeat(s, bs, axis=ax).take(np.arange(n), axis=ax)


def mx_fake_quant(x, is_bf16, qmap, axis, block_size, quant_max, pow2=False, scale_qmap=None):
    """Returns (y, scale) like MXFakeQuantFunction.forward + the `scale` buffer it fills."""
    rd = rbf if is_bf16 else (lambda a: np.asarray(a, F32))
    x = np.ascontiguousarray(x, dtype=F32)
    blocks, ax = _to_blocks(x, axis, block_size)
    with np.errstate(all="ignore"):
        amax = np.max(np.abs(blocks), axis=ax + 1)
        if not pow2:
            scale = rd((amax / F32(quant_max)).astype(F32))                                # decomposed.py:414-415
            if scale_qmap is not None:                                                     # :418-419
                scale = bf16_to_f32(vmap_bf16(f32_to_bf16(scale), scale_qmap)) if is_bf16 else vmap_f32(scale, scale_qmap)
        else:
            t = rd(amax + F32(2.0 ** -126) * (amax == 0))                                  # mx_utils.py:43-47
            e = np.floor(rd(np.log2(t).astype(F32)))
            e = rd(e - F32(math.floor(math.log2(quant_max))))                              # decomposed.py:405
            scale = rd(np.exp2(e.astype(np.float64)).astype(F32))                          # :411
        scale = np.where(scale > 0.0, scale, F32(1.0)).astype(F32)                         # :421
        se = _expand_blocks(scale, ax, block_size, x.shape[ax])
        if is_bf16:
            q = bf16_to_f32(vmap_bf16(f32_to_bf16((x / se).astype(F32)), qmap))            # quantize, decomposed.py:205-210
        else:
            q = vmap_f32((x / se).astype(F32), qmap)
        y = rd((q * se).astype(F32))                                                       # fake_quantize.py:128
    return y, scale


def group_wise_affine_fake_quant(x, is_bf16, axis, block_size, quant_min, quant_max):
    """Returns (y, scale, zero_point) like GroupWiseAffineFakeQuantFunction.forward (no scale_qmap)."""
    rd = rbf if is_bf16 else (lambda a: np.asarray(a, F32))
    x = np.ascontiguousarray(x, dtype=F32)
    blocks, ax = _to_blocks(x, axis, block_size)
    with np.errstate(all="ignore"):
        mn = np.min(blocks, axis=ax + 1)                                                   # fake_quantize.py:166-167
        mx = np.max(blocks, axis=ax + 1)
        sf = rd(rd(mx - mn) / F32(quant_max - quant_min))                                  # :169
        sf = np.where(sf > 0.0, sf, F32(1.0)).astype(F32)                                  # :170
        zp = rd(rd(rd(-mn) / sf) + F32(quant_min))                                         # :171
        se = _expand_blocks(sf, ax, block_size, x.shape[ax])
        ze = _expand_blocks(zp, ax, block_size, x.shape[ax])
        q = _clamp(np.rint(rd(rd(x / se) + ze)), F32(quant_min), F32(quant_max))           # :185
        y = rd(rd(q - ze) * se)                                                            # :188
    return y.astype(F32), sf, zp


# ---- packed block-scaled operands (OCP MX element codes + E8M0 scales) --------------------------------------
# What linear_mx / matmul_mx consume is (values, block scales) (decomposed.py:304-363).  The matrix instruction
# wants the same numbers as element codes and one exponent byte per 32 elements; this is that re-encoding,
# restated on the host so the device packer can be checked bit for bit.
MX_ELEM = {"fp8_e4m3": (0, 4, 3, 7), "fp8_e5m2": (1, 5, 2, 15), "fp6_e2m3": (2, 2, 3, 1), "fp6_e3m2": (3, 3, 2, 3),
           "fp4_e2m1": (4, 2, 1, 1)}      # name -> (hardware format id, exponent bits, mantissa bits, bias)


def mx_decode(code, fmt):
    """Element code -> float64 value (OCP MX v1.0 element formats; no Inf/NaN codes are produced by mx_encode)."""
    _, eb, mb, bias = MX_ELEM[fmt]
    code = np.asarray(code, dtype=np.int64)
    s = (code >> (eb + mb)) & 1
    e = (code >> mb) & ((1 << eb) - 1)
    m = code & ((1 << mb) - 1)
    v = np.where(e == 0, np.ldexp(m.astype(np.float64), 1 - bias - mb), np.ldexp(((1 << mb) | m).astype(np.float64), e - bias - mb))
    return np.where(s == 1, -v, v)


def mx_encode(values, fmt):
    """float values that are exactly representable in `fmt` -> element codes; raises if one is not."""
    _, eb, mb, bias = MX_ELEM[fmt]
    v = np.asarray(values, dtype=np.float64)
    table = mx_decode(np.arange(1 << (eb + mb)), fmt)          # non-negative half, increasing
    finite = table[: {"fp8_e4m3": 0x7F, "fp8_e5m2": 0x7C}.get(fmt, len(table))]     # drop the NaN / Inf codes of the 8-bit formats
    idx = np.searchsorted(finite, np.abs(v))
    idx = np.clip(idx, 0, len(finite) - 1)
    if not np.array_equal(finite[idx], np.abs(v)):
        raise ValueError(f"value not representable in {fmt}")
    return (idx | (np.signbit(v).astype(np.int64) << (eb + mb))).astype(np.uint32)


def mx_pack(values, scales, fmt, block_size=32):
    """values [rows, K], scales [rows, K / block_size] (powers of two) -> (codes uint8 [rows, K*bits/8], e8m0 uint8 [rows, K/32]).
    Element i of a row occupies bits [i*bits, (i+1)*bits) of the row, little-endian."""
    _, eb, mb, _ = MX_ELEM[fmt]
    bits = 1 + eb + mb
    values = np.asarray(values, dtype=np.float64)
    rows, K = values.shape
    codes = mx_encode(values, fmt).astype(np.uint64)
    bitpos = np.arange(K, dtype=np.uint64) * np.uint64(bits)
    out = np.zeros((rows, K * bits // 8), dtype=np.uint8)
    for b in range(bits):
        pos = bitpos + np.uint64(b)
        byte, off = (pos >> np.uint64(3)).astype(np.int64), (pos & np.uint64(7)).astype(np.uint8)
        bitv = ((codes >> np.uint64(b)) & np.uint64(1)).astype(np.uint8)
        np.bitwise_or.at(out, (np.arange(rows)[:, None], byte[None, :]), bitv << off[None, :])
    s = np.asarray(scales, dtype=np.float64)
    m, e = np.frexp(s)                                            # s = m * 2^e, m in [0.5, 1)
    if not np.all(m == 0.5):
        raise ValueError("scale is not a power of two")
    e8 = (e - 1 + 127)
    if np.any(e8 < 0) or np.any(e8 > 254):
        raise ValueError("scale outside E8M0")
    e8 = np.repeat(e8.astype(np.uint8), block_size // 32, axis=1)
    return out, e8


# ---- attention-score path with every bf16 rounding point explicit ---------------------------------------------------------
# modules/quantizable/modeling_bert.py:118, 142-158 (and the HF LLaMA eager path the LLaMA twin follows):
#     scores = qk_matmul(q, k^T)                     bf16 tensor (fp32-accumulated GEMM, ONE rounding)
#     t      = attn_scaling(scores, scaling)         bf16 x python float -> bf16 (ONE rounding of the fp32 product)
#     u      = t + mask                              bf16 + bf16 -> bf16 (ONE rounding)
#     p      = softmax(u) in fp32, then bf16         (ONE rounding; nn.Softmax on bf16 computes in fp32 as well)
#     pq     = fake-quant(p)                         value map on the bf16 pattern (av_matmul's input hook, quantize.py:128-140)
#     out    = av_matmul(pq, v)                      bf16 (fp32-accumulated GEMM, ONE rounding)
# exp and every sum are evaluated in float64 here, so this is the chain's value with exact transcendental / reduction
# arithmetic; an implementation in fp32 differs from it only where its ~1e-7 relative error straddles a bf16 rounding
# boundary -- a few elements in 10^4, each by one bf16 ULP -- whereas a missing or extra rounding point moves a large
# share of the elements.
def _rbf64(x):
    """float64 -> nearest bf16 value (as float64), through fp32 like the hardware path: the fp32 rounding is exact for
    products / sums of two bf16 values, so double rounding cannot occur for the single-operation steps below."""
    return bf16_to_f32(f32_to_bf16(np.asarray(x, dtype=np.float64).astype(np.float32))).astype(np.float64)


def scale_and_mask(scores_bits, mask_bits, scaling):
    """The softmax's input in bf16: bf16(bf16(score x scaling) + mask), each step ONE rounding of an exactly representable fp32
    result (modeling_bert.py:142-146: MulFunctional with a python float, then `+ attention_mask`).  Returns float64 values."""
    s = bf16_to_f32(scores_bits).astype(np.float64)
    t = _rbf64(s.astype(np.float32) * np.float32(scaling))
    if mask_bits is not None:
        m = bf16_to_f32(mask_bits).astype(np.float64)
        with np.errstate(over="ignore"):
            t = _rbf64(t + m)
    return t


def softmax_fq(scores_bits, mask_bits, scaling, qmap, with_interval=False):
    """scores_bits: uint16 [..., rows, cols] bf16 patterns; mask_bits: broadcastable uint16 array or None; scaling: python
    float (multiplied as fp32, like torch's bf16-tensor x scalar); qmap: uint16[65536] or None.  Returns (p_bits, pq_bits); with
    `with_interval` also the probabilities' admissible interval (softmax_interval, below) as a third element.
    Pinned to upstream's BertSelfAttention twin by tests/test_oracle_golden.py::test_attention_chain (tests/golden/attn_chain.*)."""
    t = scale_and_mask(scores_bits, mask_bits, scaling)
    mx = t.max(axis=-1, keepdims=True)
    e = np.exp(t - mx)
    p = e / e.sum(axis=-1, keepdims=True)
    p_bits = f32_to_bf16(p.astype(np.float32))
    out = p_bits, (vmap_bf16(p_bits, qmap) if qmap is not None else p_bits)
    return out + (softmax_interval(scores_bits, mask_bits, scaling),) if with_interval else out


def softmax_fq_f32(scores, mask, scaling, qmap):
    """The same chain on an fp32 model (no bf16 rounding points; the probabilities' fake-quantizer indexes the map with
    hi16 | sticky, decomposed.py:151-153): scores / mask float32 arrays.  exp and the sums in float64, ONE rounding to fp32.
    Returns (p float32, pq float32)."""
    t = (scores.astype(np.float32) * np.float32(scaling)).astype(np.float32)
    if mask is not None:
        with np.errstate(over="ignore"):
            t = (t + mask.astype(np.float32)).astype(np.float32)
    t = t.astype(np.float64)
    mx = t.max(axis=-1, keepdims=True)
    e = np.exp(t - mx)
    p = (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)
    return p, (vmap_f32(p, qmap) if qmap is not None else p)


def attention_fq(q_bits, k_bits, v_bits, mask_bits, scaling, qmap, scale_bits=None):
    """q [B,H,Sq,D], k / v [B,H,Sk,D] as uint16 bf16 patterns (already fake-quantized); returns the attention output
    [B,H,Sq,D] as bf16 patterns plus the quantized probabilities' patterns.  scale_bits: the bf16 pattern of the probabilities'
    fake-quantizer's scale (fq_bf16), None for unit scale."""
    q = bf16_to_f32(q_bits).astype(np.float64)
    k = bf16_to_f32(k_bits).astype(np.float64)
    v = bf16_to_f32(v_bits).astype(np.float64)
    with np.errstate(invalid="ignore"):
        scores = f32_to_bf16(np.einsum("bhqd,bhkd->bhqk", q, k).astype(np.float32))
    with np.errstate(invalid="ignore", over="ignore"):
        p_bits, pq_bits = softmax_fq(scores, mask_bits, scaling, qmap)
        if scale_bits is not None and qmap is not None:
            pq_bits = fq_bf16(p_bits, qmap, np.asarray(scale_bits, U16))
        pq = bf16_to_f32(pq_bits).astype(np.float64)
        out = np.einsum("bhqk,bhkd->bhqd", pq, v)
    return f32_to_bf16(out.astype(np.float32)), pq_bits


# ---- row reductions: norms, softmax backward, causal-LM loss -- fp64 restatements with an error interval ---------------------------------
# Each function below restates one row-reduction kernel's documented chain (csrc/qt_model_ops.hip, qt_softmax.hip, qt_elementwise.hip) on
# bf16 bit patterns.  Every bf16 rounding point of the chain is explicit; every sum and transcendental is evaluated in float64.  A result
# is a RowInterval per output tensor:
#     v        the float64 value in front of the chain's FIRST INEXACT rounding
#     rho      a radius any correct fp32 evaluation of that value stays within (derived in each docstring, never measured)
#     lo, hi   bf16 patterns: the images of v - rho and v + rho under the rest of the chain, which is exact and monotone once the first
#              rounding is fixed.  An element is DECIDED when lo == hi: every correct implementation writes that pattern.
# The error model (u = 2^-24, the unit roundoff of fp32):
#     sums         an fp32 sum whose terms pass through chains of at most d = 128 additions: |error| <= d u sum|t_i|.  d is a contract of
#                  these kernels: at most 64 serial additions per lane, then the lane tree and the LDS stage, with margin.  A sum with at
#                  most one non-zero term is exact (adding zeros does not round).
#     * + -        one u (relative) each; a fused multiply-add only removes a rounding
#     rsqrtf logf  4 u relative (the documented 1 ulp, doubled); 1 / x is given the same 4 u
#     __expf(a)    (2 + 1.4427 |a|) 2^-23 relative: the argument's scaling by log2(e) plus v_exp_f32
#     subnormals   softmax probabilities get an absolute 2^-126: a result in the fp32 subnormal range may be flushed to zero.  Whether the
#                  hardware path does flush there is NOT verified on hardware; the radius admits both.
#     overflow     modelled explicitly: a sum of squares with a term above the fp32 maximum is inf, its rsqrt 0.  Zeros compare without
#                  regard to sign (bf16_order maps both to 0).
U_F32 = 2.0 ** -24
SUM_DEPTH = 128
F32_MAX = float(np.finfo(np.float32).max)


class RowInterval:
    """v, rho: float64 arrays; lo, hi: uint16 bf16 patterns (NaN: 0x7FC0 in both)."""

    def __init__(self, v, rho, lo, hi):
        self.v, self.rho = np.asarray(v, np.float64), np.asarray(rho, np.float64)
        lo, hi = canon_nan16(lo), canon_nan16(hi)
        swap = bf16_order(lo) > bf16_order(hi)
        self.lo, self.hi = np.where(swap, hi, lo).astype(U16), np.where(swap, lo, hi).astype(U16)

    def rows(self, sel):
        return RowInterval(self.v[sel], self.rho[sel], self.lo[sel], self.hi[sel])

    @property
    def nan(self):
        return (self.lo == 0x7FC0) | (self.hi == 0x7FC0)

    @property
    def decided(self):
        return (bf16_order(self.lo) == bf16_order(self.hi)) & ~self.nan

    def decided_share(self):
        """Share of the finite elements whose pattern the oracle fixes."""
        fin = ~self.nan
        return float(self.decided[fin].mean()) if fin.any() else 1.0

    def distance(self, got_bits):
        """Per element: 0 inside [lo, hi] (in bf16 value order, -0 == +0), else the number of bf16 steps outside; NaN must meet NaN
        (a mismatch counts as 65536)."""
        got = canon_nan16(got_bits)
        k, klo, khi = bf16_order(got), bf16_order(self.lo), bf16_order(self.hi)
        d = np.maximum(np.maximum(klo - k, k - khi), 0)
        gnan = got == 0x7FC0
        return np.where(gnan | self.nan, np.where(gnan & self.nan, 0, 65536), d)

    def report(self, got_bits):
        d = self.distance(got_bits)
        return f"decided share {self.decided_share():.4f}, worst distance from the interval {int(d.max())} bf16 steps, {int((d > 0).sum())} of {d.size} outside"


def bf16_order(bits):
    """bf16 patterns -> int32 keys in value order; -0 and +0 share key 0.  (NaN patterns get keys beyond the infinities.)"""
    b = np.asarray(bits, dtype=U16).astype(np.int32)
    return np.where(b < 0x8000, b, -(b & 0x7FFF))


def _b64(bits):
    return bf16_to_f32(bits).astype(np.float64)


def _bf16_of(x64):
    """float64 -> bf16 pattern, ONE rounding to nearest even.  (Through fp32 would round twice; for an interval end point the difference
    could only move the end by a pattern where v +- rho sits within 2^-29 relative of a bf16 tie, so round once, from the fp64 value:
    RNE on the fp64 image truncated to sticky.)"""
    x64 = np.asarray(x64, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x64.astype(F32)                                       # RNE to fp32 ...
        # ... made sticky: where fp32 rounding was inexact and landed exactly on a bf16 tie, nudge toward the true value
        tie = (f.view(U32) & U32(0xFFFF)) == U32(0x8000)
        f64 = f.astype(np.float64)
        adj = np.where(tie & np.isfinite(f64) & (f64 != x64), np.where((np.abs(x64) > np.abs(f64)), 1, -1), 0)
        f = (f.view(U32).astype(np.int64) + adj).astype(U32).view(F32)
    return f32_to_bf16(f)


def _sum_radius(abs_terms, axis=-1, keepdims=True):
    """d u sum|t_i| -- and 0 where at most one term is non-zero."""
    a = np.asarray(abs_terms, np.float64)
    r = SUM_DEPTH * U_F32 * a.sum(axis=axis, keepdims=keepdims)
    return np.where((a != 0).sum(axis=axis, keepdims=keepdims) <= 1, 0.0, r)


def _interval(v, rho, then=None):
    """RowInterval of bf16(v +- rho); `then` maps a bf16 pattern array through the (exact, monotone) rest of the chain."""
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = _bf16_of(v - rho), _bf16_of(v + rho)
    if then is not None:
        lo, hi = then(lo), then(hi)
    return RowInterval(v, rho, lo, hi)


def bf16_add(a_bits, b_bits):
    """torch's bf16 + bf16: the fp32 sum (correctly rounded), then ONE rounding to bf16 -- what the residual variants write to `sum`."""
    with np.errstate(over="ignore", invalid="ignore"):
        return f32_to_bf16(bf16_to_f32(a_bits) + bf16_to_f32(b_bits))


def _bf16_mul(a_bits, b_bits):
    """bf16(a * b): the product of two bf16 values is exact in fp32 (16 significant bits), so this is one rounding."""
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return f32_to_bf16(bf16_to_f32(a_bits) * bf16_to_f32(b_bits))


def _sq_sum_f32(sq_terms):
    """The fp32 fate of a sum of non-negative fp64 terms: (value, certain_inf, maybe_inf).  A term or a total beyond the fp32 maximum
    (with the sum's own error margin) is certainly inf; a total within that margin of the maximum may be either."""
    s = sq_terms.sum(axis=-1, keepdims=True)
    margin = SUM_DEPTH * U_F32
    with np.errstate(invalid="ignore"):
        certain = (sq_terms.max(axis=-1, keepdims=True) > F32_MAX) | (s * (1 - margin) > F32_MAX)
        maybe = ~certain & (s * (1 + margin) > F32_MAX)
    return np.where(certain, np.inf, s), certain, maybe


def rmsnorm(x_bits, w_bits, eps, res_bits=None):
    """LlamaRMSNorm on bf16 rows [rows, cols] (csrc/qt_model_ops.hip):  s = bf16(x + res) (optional);  r = rsqrt(mean(s^2) + eps) in
    fp32;  h = bf16(s * r);  y = bf16(w * h).  Returns (y: RowInterval, sum_bits or None).

    First inexact rounding: h.  v = s * r.  Radius: the squares s_i^2 are exact in fp32; their sum has relative error d u (all terms are
    non-negative); 1 / cols, the product with it and the addition of eps add one u each, so the rsqrt's argument is within (d + 3) u
    relative and its result within (d + 3) u / 2 + 4 u; the product s * r adds u.  rho = |v| ((d + 3) / 2 + 5 + 1) u -- one further u for
    the second-order terms -- plus 2^-149 (an fp32 product in the subnormal range rounds absolutely; the same 2^-149 per square
    below 2^-126 moves the mean square by at most that much, r by r^3 2^-150).  After h the chain is
    y = bf16(w * h): an exact product, one rounding, monotone in h for the sign of w.
    Overflow: a square beyond the fp32 maximum makes the sum inf, r = 0 and h = s * 0 = +-0 (NaN where s is inf); a row whose sum of
    squares lies within d u of the maximum admits both fates."""
    s_bits = np.asarray(x_bits, U16) if res_bits is None else bf16_add(x_bits, res_bits)
    s = _b64(s_bits)
    cols = s.shape[-1]
    with np.errstate(all="ignore"):
        ss, _, maybe = _sq_sum_f32(s * s)
        r = 1.0 / np.sqrt(ss / cols + float(F32(eps)))
        v = s * r
        rho = np.abs(v) * (((SUM_DEPTH + 3) / 2 + 6) * U_F32 + 0.5 * 2.0 ** -149 * r * r) + 2.0 ** -149
        rho = np.where(np.isnan(v), np.nan, np.where(r == 0, 0.0, rho))
    w = np.broadcast_to(np.asarray(w_bits, U16), s.shape)
    y = _interval(v, rho, then=lambda h: _bf16_mul(w, h))
    if maybe.any():                                                # the sum may or may not have overflowed: admit y = +-0 as well
        zero = np.zeros_like(y.lo)
        m = np.broadcast_to(maybe, s.shape) & ~y.nan
        y = RowInterval(y.v, y.rho, np.where(m & (bf16_order(y.lo) > 0), zero, y.lo), np.where(m & (bf16_order(y.hi) < 0), zero, y.hi))
    return y, (None if res_bits is None else s_bits)


class LayerNormResult(NamedTuple):
    """What layernorm() returns; the statistics are float64, one per row."""
    y: RowInterval
    mean: np.ndarray            # the fp64 mean, admissible within +- rho_mean
    rho_mean: np.ndarray
    rstd: np.ndarray            # the fp64 rstd, admissible within [rstd_lo, rstd_hi]
    rstd_lo: np.ndarray
    rstd_hi: np.ndarray
    sum_bits: Optional[np.ndarray]      # bf16(x + res), None without a residual


def layernorm(x_bits, w_bits, b_bits, eps, res_bits=None):
    """torch's native_layer_norm on bf16 rows (csrc/qt_model_ops.hip layernorm_kernel, csrc/qt_elementwise.hip ln_train_fwd_kernel):
    s = bf16(x + res) (optional);  mean = sum(s) / cols;  rstd = rsqrt(sum((s - mean)^2) / cols + eps);  y = bf16(w * (rstd * (s - mean))
    + b), everything in front of that one rounding in fp32.  Returns a LayerNormResult.

    First inexact rounding: y itself (v = w rstd (s - mean) + b).  Radius, step by step:
      mean   the sum of the row: d u sum|s_i|; the division by cols (exact in fp32) one u:  rho_mean = d u mean|s_i| + 2 u |mean|
      var    with the computed mean m^, sum (s_i - m^)^2 = sum (s_i - mean)^2 + cols (m^ - mean)^2 exactly, so the sum the kernel forms is
             cols (var + delta^2), 0 <= delta <= rho_mean; each term carries 2 u (the subtraction, squared) + u (the square), the sum
             d u, the product with the rounded 1 / cols two u, the addition of eps one:  the rsqrt's argument lies in
             [(var + eps) (1 - (d + 6) u), (var + rho_mean^2 + eps) (1 + (d + 6) u)]  -+ 2^-149 (squares in the subnormal range)
      rstd   4 u relative around the rsqrt of that:  [rstd_lo, rstd_hi]  (rows with |mean| >> std, constant rows above all, get a wide
             interval here: rho_mean^2 is not small against var + eps.  They are the ill-conditioned rows.)
      y      |s - mean| =: A is known to rho_mean; the difference, the two products carry 3 u (4 with margin):  the product rstd (s - m^)
             lies in [P_lo, P_hi] = [rstd_lo (A - rho_mean), rstd_hi (A + rho_mean)] (1 -+ 4 u) (P_lo with rstd_hi where A < rho_mean);
             rho = |w| max(P_hi - P, P - P_lo) + u (|w| P_hi + |b|), the last term for the final addition.
    Overflow: a squared difference beyond the fp32 maximum makes the variance inf and rstd = 0, so y = bf16(w * 0 + b) = b exactly."""
    s_bits = np.asarray(x_bits, U16) if res_bits is None else bf16_add(x_bits, res_bits)
    s = _b64(s_bits)
    cols = s.shape[-1]
    w, b = _b64(np.broadcast_to(np.asarray(w_bits, U16), s.shape)), _b64(np.broadcast_to(np.asarray(b_bits, U16), s.shape))
    u, d = U_F32, SUM_DEPTH
    with np.errstate(all="ignore"):
        mean = s.sum(-1, keepdims=True) / cols
        rho_mean = _sum_radius(np.abs(s)) / cols + 2 * u * np.abs(mean)
        diff = s - mean
        _, certain, maybe = _sq_sum_f32((np.abs(diff) + rho_mean) ** 2)         # (the overflow question is asked of the largest admissible terms)
        var = (diff * diff).sum(-1, keepdims=True) / cols
        e = float(F32(eps))
        tiny = 2.0 ** -149                                         # a square below 2^-126 rounds absolutely: 2^-149 per term, so per mean
        m_lo, m_hi = (var + e) * (1 - (d + 6) * u) - tiny, (var + rho_mean ** 2 + e) * (1 + (d + 6) * u) + tiny
        rstd = 1.0 / np.sqrt(var + e)
        rstd_lo, rstd_hi = (1 - 4 * u) / np.sqrt(m_hi), (1 + 4 * u) / np.sqrt(m_lo)
        rstd, rstd_lo, rstd_hi = (np.where(certain, 0.0, t) for t in (rstd, rstd_lo, rstd_hi))
        rstd_lo = np.where(maybe, 0.0, rstd_lo)
        A = np.abs(diff)
        P = rstd * A
        P_hi = rstd_hi * (A + rho_mean) * (1 + 4 * u)
        P_lo = np.where(A >= rho_mean, rstd_lo * (A - rho_mean) * (1 - 4 * u), rstd_hi * (A - rho_mean) * (1 + 4 * u))
        v = w * (rstd * diff) + b
        rho = np.abs(w) * np.maximum(P_hi - P, P - P_lo) + u * (np.abs(w) * P_hi + np.abs(b))
        rho = np.where(np.isnan(v), np.nan, np.where(np.broadcast_to(certain, s.shape), 0.0, rho))
    return LayerNormResult(_interval(v, rho), mean[..., 0], rho_mean[..., 0], rstd[..., 0], rstd_lo[..., 0], rstd_hi[..., 0],
                           None if res_bits is None else s_bits)


def layernorm_backward(dy_bits, x_bits, w_bits, mean, rstd):
    """torch's native_layer_norm_backward on bf16 rows [rows, cols] from GIVEN fp32 statistics (csrc/qt_elementwise.hip
    ln_train_bwd_kernel):  xh = (x - mean) rstd;  g = dy w;  c1 = mean(g);  c2 = mean(g xh);  dx = bf16(rstd (g - c1 - xh c2));
    dgamma = bf16(sum_rows dy xh);  dbeta = bf16(sum_rows dy).  Returns (dx, dgamma, dbeta) as RowIntervals.

    First inexact rounding: each output's own.  Radii: xh carries 2 u; g is an exact product.  s1 = sum g: d u sum|g|.  s2 = sum g xh:
    3 u per term and d u for the sum: (d + 3) u sum|g xh|.  c1, c2: two u each for 1 / cols and the product:
    rho_c = rho_s / cols + 2 u |c|.  The bracket g - c1 - xh c2 then errs by rho_c1 + |xh| rho_c2 + 4 u (|g| + |c1| + |xh c2|) (the product
    xh c2 with xh's two u, both subtractions), the product with rstd adds u:
        rho_dx = rstd (rho_c1 + |xh| rho_c2 + 4 u (|g| + |c1| + |xh c2|)) + u |dx|.
    dgamma: terms dy xh with 3 u each, sum over the rows d u: (d + 3) u sum|dy xh|;  dbeta: exact terms, d u sum|dy|."""
    dy, x = _b64(dy_bits), _b64(x_bits)
    w = _b64(np.broadcast_to(np.asarray(w_bits, U16), x.shape))
    mean = np.asarray(mean, F32).astype(np.float64).reshape(-1, 1)
    rstd = np.asarray(rstd, F32).astype(np.float64).reshape(-1, 1)
    cols = x.shape[-1]
    u, d = U_F32, SUM_DEPTH
    with np.errstate(all="ignore"):
        xh = (x - mean) * rstd
        g = dy * w
        c1, c2 = g.sum(-1, keepdims=True) / cols, (g * xh).sum(-1, keepdims=True) / cols
        rho_c1 = _sum_radius(np.abs(g)) / cols + 2 * u * np.abs(c1)
        rho_c2 = (d + 3) * u * np.abs(g * xh).sum(-1, keepdims=True) / cols + 2 * u * np.abs(c2)
        v = rstd * (g - c1 - xh * c2)
        rho = rstd * (rho_c1 + np.abs(xh) * rho_c2 + 4 * u * (np.abs(g) + np.abs(c1) + np.abs(xh * c2))) + u * np.abs(v) + 2.0 ** -149
        t = dy * xh
        vg, rg = t.sum(0), (d + 3) * u * np.abs(t).sum(0) + 2.0 ** -149
        vb, rb = dy.sum(0), _sum_radius(np.abs(dy), axis=0, keepdims=False)
    return _interval(v, rho), _interval(vg, rg), _interval(vb, rb)


def softmax_backward(dp_bits, p_bits, scaling):
    """torch's _softmax_backward_data on bf16 rows, then the scaling's backward (csrc/qt_softmax.hip softmax_bwd_kernel):
    d1 = bf16((dP - sum(dP P)) P) in fp32;  ds = bf16(d1 * scaling), the product rounded to fp32 first (scaling is an fp32 number).
    Returns ds as a RowInterval.

    First inexact rounding: d1.  v = (dP - dot) P.  The products dP_i P_i are exact in fp32, the dot product errs by
    rho_dot = d u sum|dP_i P_i| (0 for a one-hot row: one non-zero term).  The subtraction and the product add one u each:
        rho = |P| rho_dot + 2 u |v|  (times 1 + 2^-20 for the second-order terms) + 2^-149.
    After d1 the chain is the deterministic pair of roundings fp32(d1 * scaling) -> bf16, monotone in d1 (for scaling > 0)."""
    dp, p = _b64(dp_bits), _b64(p_bits)
    sc = F32(scaling)
    with np.errstate(all="ignore"):
        t = dp * p
        dot = t.sum(-1, keepdims=True)
        v = (dp - dot) * p
        rho = (np.abs(p) * _sum_radius(np.abs(t)) + 2 * U_F32 * np.abs(v)) * (1 + 2.0 ** -20)
        rho = np.where(rho == 0, 0.0, rho + 2.0 ** -149)

    def then(d1):
        with np.errstate(all="ignore"):
            return f32_to_bf16(bf16_to_f32(d1) * sc)
    return _interval(v, rho, then=then)


def softmax_interval(scores_bits, mask_bits, scaling):
    """The probabilities of softmax_fq with their admissible interval (csrc/qt_softmax.hip softmax_fq_kernel):
    t = bf16(bf16(score x scaling) + mask) is bit-defined, so is the row maximum;  a = t - max;  e = __expf(a);  p = bf16(e * (1 / sum e)).

    First inexact rounding: p.  v = exp(a) / sum exp(a).  Per term, rel_i = (2 + 1.4427 |a_i|) 2^-23 + u |a_i| (the subtraction t - max
    of two bf16 values can round).  The sum errs by its terms' errors, sum_j e_j rel_j, and by d u; relative to the sum that is the
    p-weighted mean of rel_j, plus d u.  The reciprocal 4 u, the product u:
        rho = v (rel_i + sum_j v_j rel_j + (d + 5) u) + 2^-126,
    the absolute term for a flush of a subnormal exponential or product (not verified on hardware, see above).  Vectors the kernel skips
    (all eight logits more than 110 below the maximum) hold values below 2^-158: zero in bf16 either way.
    Where a < -104.5 the exponential with its relative error lies below 2^-150, half the smallest fp32 subnormal: every fp32 evaluation,
    flushing or not, returns 0, the sum is at least 1 (the maximum's own term), so p = 0 exactly: v = 0, rho = 0 there."""
    t = scale_and_mask(scores_bits, mask_bits, scaling)
    with np.errstate(all="ignore"):
        a = t - t.max(axis=-1, keepdims=True)
        e = np.exp(a)
        v = e / e.sum(axis=-1, keepdims=True)
        rel = np.where(np.isfinite(a), (2 + 1.4427 * np.abs(a)) * 2.0 ** -23 + U_F32 * np.abs(a), 0.0)
        rho = v * (rel + (v * rel).sum(axis=-1, keepdims=True) + (SUM_DEPTH + 5) * U_F32) + 2.0 ** -126
        gone = a < -104.5                                          # (false for NaN)
        v = np.where(gone, 0.0, v)
        rho = np.where(np.isnan(v), np.nan, np.where(gone, 0.0, rho))
        iv = _interval(v, rho)
        neg = bf16_order(iv.lo) < 0                      # a probability is never negative: e >= 0 and 1 / sum > 0
    return RowInterval(iv.v, iv.rho, np.where(neg & ~iv.nan, U16(0), iv.lo), iv.hi)


def causal_lm_nll(logits_bits, labels, ignore_index=-100):
    """transformers' ForCausalLMLoss on bf16 logits [B, S, V] (csrc/qt_model_ops.hip nll_rows_kernel / nll_mean_kernel): position s is
    scored against labels[s + 1] (the last position of a sequence, an ignored or out-of-range label: not scored);
    loss = (max + log sum exp(x - max)) - x[label] in fp32;  the result is the mean over the scored positions (NaN when there are none).
    Returns (loss [B, S] float64, rho [B, S], scored [B, S] bool, mean, rho_mean); unscored positions hold NaN.

    Radius: the kernel keeps a running maximum, so a term exp(x_j - max) is a product of up to K exponentials whose (non-positive)
    arguments add up to x_j - max: K <= ceil(V / 2048) + 8 (a lane's maximum updates, six lane-tree steps, the LDS stage).
    rel_j = (2 K + 1.4427 |a_j|) 2^-23 + (K + |a_j|) u.  The sum S: p-weighted mean of rel_j plus d u =: rel_S.  logf: 4 u |log S|, and
    log(S (1 + rel_S)) - log S <= 2 rel_S.  The two additions one u each:
        rho = 2 rel_S + 4 u |log S| + u |max + log S| + u |loss| + 2^-149.
    The mean: rho_mean = (sum rho_i + d u sum|loss_i|) / n + u |mean|."""
    x = _b64(logits_bits)
    B, S, V = x.shape
    labels = np.asarray(labels, np.int64)
    lab = np.full((B, S), ignore_index, np.int64)
    lab[:, :-1] = labels[:, 1:]
    scored = (lab != ignore_index) & (lab >= 0) & (lab < V)
    K = -(-V // 2048) + 8
    u = U_F32
    with np.errstate(all="ignore"):
        mx = x.max(-1, keepdims=True)
        a = x - mx
        e = np.exp(a)
        Ssum = e.sum(-1, keepdims=True)
        p = e / Ssum
        rel = np.where(np.isfinite(a), (2 * K + 1.4427 * np.abs(a)) * 2.0 ** -23 + (K + np.abs(a)) * u, 0.0)
        rel_S = ((p * rel).sum(-1, keepdims=True) + SUM_DEPTH * u)[..., 0]
        logS, mx = np.log(Ssum)[..., 0], mx[..., 0]
        xl = np.take_along_axis(x, np.where(scored, lab, 0)[..., None], -1)[..., 0]
        loss = (mx + logS) - xl
        rho = 2 * rel_S + 4 * u * np.abs(logS) + u * np.abs(mx + logS) + u * np.abs(loss) + 2.0 ** -149
        loss, rho = np.where(scored, loss, np.nan), np.where(scored, rho, np.nan)
        n = int(scored.sum())
        if n == 0:
            return loss, rho, scored, float("nan"), float("nan")
        mean = loss[scored].sum() / n
        rho_mean = (rho[scored].sum() + SUM_DEPTH * u * np.abs(loss[scored]).sum()) / n + u * abs(mean)
    return loss, rho, scored, float(mean), float(rho_mean)


# ---- elementwise launches: rotary, SiLU * up, GELU (csrc/qt_model_ops.hip) -----------------------------------------------------------------
def rope(x_bits, cos_bits, sin_bits, inner_qmap=None, out_qmap=None):
    """The rotary embedding on bf16 patterns x [B, S, H, D] with tables cos / sin [B, S, D] (HF's apply_rotary_pos_emb on bf16 tensors;
    rope_one / rope_fq_token of csrc/qt_model_ops.hip):

        y = bf16( fq_inner(bf16(x * cos)) + bf16(rotate_half(x) * sin) ),   rotate_half(x) = cat(-x[D/2:], x[:D/2]),

    then out_qmap (a value map, uint16[65536]) applied to y.  inner_qmap is the value map PT2E graphs put on the earlier operand of the
    add.  cos_bits None: no rotation, y = x.

    Bit for bit, no interval: the product of two bf16 values has 16 significant bits and is exact in fp32 (in the subnormal range too:
    it is a multiple of 2^-149 wherever it is at least that large, and below that one correctly rounded fp32 product), the fp32 sum of
    two bf16 values is correctly rounded, and each is rounded once more to bf16 -- numpy float32 arithmetic performs exactly these
    roundings, keeps subnormals and follows IEEE for inf * 0 and inf - inf.  Returns bf16 patterns in the order of x, NaN canonical."""
    x_bits = np.asarray(x_bits, U16)
    if cos_bits is None:
        y = canon_nan16(x_bits)
    else:
        half = x_bits.shape[-1] // 2
        x = bf16_to_f32(x_bits)
        c, s = bf16_to_f32(cos_bits)[:, :, None, :], bf16_to_f32(sin_bits)[:, :, None, :]
        with np.errstate(all="ignore"):
            a = f32_to_bf16(x * c)
            if inner_qmap is not None:
                a = vmap_bf16(a, inner_qmap)
            rot = np.concatenate([-x[..., half:], x[..., :half]], axis=-1)
            b = f32_to_bf16(rot * s)
            y = f32_to_bf16(bf16_to_f32(a) + bf16_to_f32(b))
    if out_qmap is not None:
        y = vmap_bf16(y, out_qmap)
    return canon_nan16(y)


LN_F32_MAX = math.log(F32_MAX)              # 88.7228...: expf of anything above is +inf in fp32
SILU_U = 12                                 # radius of the SiLU quotient in units of u (derived in silu_mul's docstring)
ERFF_U = 8                                  # absolute error of erff in units of u |erf| (gelu's docstring)

_ELEMENTWISE_TABLES = {}


def _silu_table():
    """Per gate pattern: (v, rho, lo, hi) of s = bf16(g / (1 + expf(-g)))."""
    if "silu" not in _ELEMENTWISE_TABLES:
        with np.errstate(all="ignore"):
            g = _b64(all_bf16_patterns())
            v = g / (1.0 + np.exp(-g))
            rho = SILU_U * U_F32 * np.abs(v) + 2.0 ** -149
            over = -g > LN_F32_MAX                                 # expf(-g) = +inf: the quotient is g / inf
            v = np.where(over, np.where(np.isinf(g), np.nan, -0.0), v)
            rho = np.where(over | (v == 0) | np.isinf(v), 0.0, rho)
            rho = np.where(np.isnan(v), np.nan, rho)
        iv = _interval(v, rho)
        _ELEMENTWISE_TABLES["silu"] = (v, rho, iv.lo, iv.hi)
    return _ELEMENTWISE_TABLES["silu"]


def silu_mul(gate_bits, up_bits):
    """SiLU(gate) * up on bf16 patterns (silu_mul_kernel; HF's LlamaMLP act_fn(gate) * up on bf16 tensors):

        s = bf16(g / (1 + expf(-g)));   y = bf16(s * up).

    First (and only) inexact rounding: s.  v = g / (1 + e^-g) in fp64.  Radius, with the conventions of the error model above U_F32
    (u = 2^-24; a documented bound in ulp counts 2 u per ulp):
        expf      documented 1 ulp, doubled as for rsqrtf and logf: 4 u relative.  Its argument -g is exact.
        1 + e     e's error enters the sum with weight e / (1 + e) <= 1: at most 4 u; the addition rounds once: u.
        g / (.)   the documented bound of fp32 division without the correctly-rounded option is 2.5 ulp = 5 u; one more u as margin.
        second-order terms: u.
    rho = 12 u |v| + 2^-149 (a quotient in the fp32 subnormal range rounds absolutely).  A flush of such a quotient to zero is NOT
    admitted: the torch chain this restates keeps it.
    Overflow: for -g > ln(F32_MAX) = 88.72 expf returns +inf, 1 + inf = inf and g / inf is exactly -0 (fp64 alone says -2.4e-37 at
    g = -89); g = -inf gives -inf / inf = NaN.  No bf16 value lies between 88.5 and 89, and e^88.5 = 2.7e38 is a factor 1.25 below the
    fp32 maximum, so which side a gate falls on does not depend on expf's error.  g = +inf: e = 0, s = inf.  v == 0 is exact (rho 0).
    After s the chain is y = bf16(s * up): an exact product, one rounding, monotone in s for the sign of up.
    Returns the RowInterval of y (v, rho: those of s)."""
    gate_bits, up_bits = np.asarray(gate_bits, U16), np.asarray(up_bits, U16)
    v, rho, lo, hi = _silu_table()
    return RowInterval(v[gate_bits], rho[gate_bits], _bf16_mul(lo[gate_bits], up_bits), _bf16_mul(hi[gate_bits], up_bits))


def _gelu_table():
    if "gelu" not in _ELEMENTWISE_TABLES:
        with np.errstate(invalid="ignore"):
            x = _b64(all_bf16_patterns())
        fin = np.isfinite(x)
        c = float(F32(math.sqrt(0.5)))                             # the kernel's constant, rounded to fp32
        t = np.where(fin, x, 0.0) * c
        erf = np.array([math.erf(a) for a in t])
        with np.errstate(all="ignore"):
            erf = np.where(fin, erf, np.where(np.isnan(x), np.nan, np.sign(x)))
            derf = np.where(fin, 2.0 / math.sqrt(math.pi) * np.exp(-t * t), 0.0)
            v = (x * 0.5) * (1.0 + erf)
            e_abs = U_F32 * (ERFF_U * np.abs(erf) + np.abs(t) * derf + np.abs(1.0 + erf))
            rho = np.where(fin, np.abs(x * 0.5) * e_abs + 2 * U_F32 * np.abs(v) + 2.0 ** -149, 0.0)
            rho = np.where(np.isnan(v), np.nan, np.where(x == 0, 0.0, rho))
        iv = _interval(v, rho)
        _ELEMENTWISE_TABLES["gelu"] = (v, rho, iv.lo, iv.hi)
    return _ELEMENTWISE_TABLES["gelu"]


def gelu(x_bits):
    """The erf GELU on bf16 patterns (gelu_kernel; torch's GELU on a bf16 tensor):  y = bf16((x * 0.5) * (1 + erff(x * sqrt(1/2)))),
    one rounding to bf16 at the end.  v = (x / 2)(1 + erf(x c)) in fp64 with c the fp32 value of sqrt(1/2), as the kernel has it.

    Radius.  1 + erff cancels for negative x (erf -> -1), so the error of erff enters ABSOLUTELY, times |x / 2|:
        t = x * c           one rounding: u relative; it moves erf by |t| erf'(t) u, erf'(t) = 2 / sqrt(pi) e^(-t^2)
        erff(t)             a bound of 4 ulp (twice the 2 ulp commonly documented for erff, the doubling of the error model above):
                            8 u |erf(t)|
        1 + erf             one rounding: u |1 + erf|
      so |error of (1 + erff)| <= u (8 |erf| + |t| erf'(t) + |1 + erf|) =: E, and
        rho = |x / 2| E + 2 u |v| + 2^-149
    (x * 0.5 is exact; the last product rounds once, one further u for the second-order terms; a product in the fp32 subnormal range
    rounds absolutely).  x = 0: exactly 0.  x = +inf: inf * 2 = inf.  x = -inf: -inf * 0 = NaN (torch's GELU gives the same).  For
    x <= -5.6 or so the interval contains both signs of zero and the kernel's -0 (erff = -1 exactly) is inside it.
    The elements the radius cannot decide are the negative tail, where 8 u is not small against 1 + erf."""
    x_bits = np.asarray(x_bits, U16)
    v, rho, lo, hi = _gelu_table()
    return RowInterval(v[x_bits], rho[x_bits], lo[x_bits], hi[x_bits])


# ---- the attention cores: fused QK^T, scaling, mask, softmax, fq_P, P.V (csrc/qt_attention.hip, qt_attention_rows.hip, qt_attention_fp8.hip)
class AttentionIntervals(NamedTuple):
    """What attention_interval() returns."""
    out: RowInterval            # O, [B, H, Sq, D]
    probs: RowInterval          # P' = fq_P(P), [B, H, Sq, Sk]
    amax: RowInterval           # the observer's amax: the largest P in front of fq_P, shape (1,)
    pv_exact: np.ndarray        # bool [B, H, Sq]: the P'.V sums of the row carry no radius (exact in fp32 in any order)


ATTENTION_KERNELS = ("online", "strip", "strip_fp8")


def _lowbit(x):
    """The weight of the lowest set bit of |x| (float64); inf for 0 and for non-finite x.  Every x is an integer multiple of it."""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x) & (x != 0)
    m, e = np.frexp(np.where(ok, np.abs(x), 1.0))
    M = (m * 2.0 ** 53).astype(np.int64)
    return np.where(ok, np.ldexp((M & -M).astype(np.float64), e - 53), np.inf)


def _sums_exact_in_f32(abs_sum, granule):
    """A sum whose terms are integer multiples of `granule` and whose absolute values add up to abs_sum: every partial sum, in any order,
    is a multiple of the granule of magnitude <= abs_sum, so it has at most 24 significant bits -- exact in fp32 -- when
    abs_sum <= 2^24 granule."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(granule), abs_sum <= 2.0 ** 24 * granule, True)


def attention_probs_interval(t, kernel):
    """The probabilities of one attention core from its bit-defined logits t = bf16(bf16(S x scaling) + mask) (float64, [..., Sk]), with
    the admissible interval of p = bf16(exp(t - max) / sum): v = exp(a) / sum exp(a), a = t - max, exp and the sum in float64.  The error
    model is softmax_interval's (U_F32, SUM_DEPTH, the __expf term, the 2^-126 allowance); the radius follows how the kernel forms the sum.

    kernel = "strip" (and "strip_fp8", the same softmax) -- qt_attention_rows.hip:249-277, qt_attention_fp8.hip:263-291 and the
      probability at rows:306 / fp8:318.  The whole
      strip is in registers, the maximum is final before any exponential: e_i = exp2((t_i - max) * log2e) once per logit (the subtraction
      of two bf16 values rounds: u |a|; the product with log2e and v_exp_f32: the __expf term), so rel_i = (2 + 1.4427 |a_i|) 2^-23 + u |a_i|.
      The sum: at most 64 serial additions per lane and accumulator (two accumulators, 8 blocks x 4 tiles x 2), their sum, two shuffles
      and the other key group's half: 68 <= d = SUM_DEPTH.  1 / sum: 4 u; e * inv: u.
          rho = v (rel_i + sum_j v_j rel_j + (d + 5) u) + 2^-126                          (softmax_interval's radius, unchanged)
    kernel = "online" -- qt_attention.hip:302-338 (pass 1) and :361 (pass 2).  Pass 1 walks 64-key tiles with a running maximum:
      l = l * __expf(m - ref) + part, part = sum over the tile of __expf(t - ref), ref = the maximum so far.  A term's exponential
      therefore is a PRODUCT of up to K exponentials whose non-positive arguments telescope: |t - ref| + sum |m_i - m_i+1| = |t - max|.
      Only their count grows: K = 1 + the number of tiles at which the row's running maximum rises (__expf(0) = 1 and l * 1 are
      exact), so rel'_j = (2 K + 1.4427 |a_j|) 2^-23 + u |a_j| for the SUM's terms.  The sum's depth: 16 additions per lane and tile, two
      shuffles, and one product and one addition per tile: d' = SUM_DEPTH + 2 ntiles.  Pass 2 evaluates __expf(t - max) * (1 / l) with
      the final maximum: the element's own factor is rel_i with ONE exponential, 1 / l: 4 u, the product u.
          rho = v (rel_i + sum_j v_j rel'_j + (d' + 5) u) + 2^-126
      Skipped key tiles (qt_attention.hip:240-299) hold logits <= -1e30 for every row of the workgroup: their exponentials are exactly 0
      counted or not, unless the row has no other key -- and then the kernel counts every tile again (:335-336).
    Where a < -104.5 every fp32 evaluation gives exactly 0 (softmax_interval); a row holding a NaN or a +inf logit, and a row of -inf
    logits only (inf - inf), is NaN in every element, as torch's softmax gives.  A row of equal finite logits (all keys at the bf16
    minimum: fully masked) is the uniform row over all Sk keys.  Returns the RowInterval of p (lo >= 0)."""
    if kernel not in ATTENTION_KERNELS:
        raise ValueError(f"kernel must be one of {ATTENTION_KERNELS}")
    t = np.asarray(t, np.float64)
    Sk = t.shape[-1]
    with np.errstate(all="ignore"):
        a = t - t.max(axis=-1, keepdims=True)
        e = np.exp(a)
        s = e.sum(axis=-1, keepdims=True)
        v = e / s
        fin = np.isfinite(a)
        absa = np.where(fin, np.abs(a), 0.0)
        rel = np.where(fin, (2 + 1.4427 * absa) * 2.0 ** -23 + U_F32 * absa, 0.0)
        if kernel == "online":
            ntiles = -(-Sk // 64)
            pad = np.full(t.shape[:-1] + (ntiles * 64 - Sk,), -np.inf)
            tm = np.concatenate([t, pad], axis=-1).reshape(t.shape[:-1] + (ntiles, 64)).max(axis=-1)
            run = np.maximum.accumulate(tm, axis=-1)
            K = 1 + (run[..., 1:] > run[..., :-1]).sum(axis=-1, keepdims=True)
            rel_sum = np.where(fin, (2 * K + 1.4427 * absa) * 2.0 ** -23 + U_F32 * absa, 0.0)
            depth = SUM_DEPTH + 2 * ntiles
        else:
            rel_sum, depth = rel, SUM_DEPTH
        rho = v * (rel + (v * rel_sum).sum(axis=-1, keepdims=True) + (depth + 5) * U_F32) + 2.0 ** -126
        gone = a < -104.5
        v, rho = np.where(gone, 0.0, v), np.where(gone, 0.0, rho)
        nanrow = np.broadcast_to(np.isnan(s), v.shape)
        v, rho = np.where(nanrow, np.nan, v), np.where(nanrow | np.isnan(v), np.nan, rho)
        iv = _interval(v, rho)
        neg = bf16_order(iv.lo) < 0
    return RowInterval(iv.v, iv.rho, np.where(neg & ~iv.nan, U16(0), iv.lo), iv.hi)


def _prob_fq(qmap, scale_bits):
    """fq_P on bf16 patterns: identity, the value map, or the map between bf16(p / s) and bf16(. * s)."""
    if qmap is None:
        return lambda bits: canon_nan16(bits)
    if scale_bits is None:
        return lambda bits: canon_nan16(vmap_bf16(bits, qmap))
    return lambda bits: canon_nan16(fq_bf16(bits, qmap, np.asarray(scale_bits, U16)))


def _image_of_interval(table, lo, hi):
    """The image of the pattern interval [lo, hi] (non-negative bf16 patterns, or NaN in both) under a map given as a table over the
    patterns 0 .. 0x7F80: (smallest, largest) mapped pattern in value order over EVERY pattern in between.  For a monotone map that is
    (table[lo], table[hi]); the reference's maps are monotone up to artefacts of their bf16 arithmetic (fp4_e2m1 sends 0x3E7F, just
    below 0.25, to 0.5 and 0.25 to 0), and this is the exact image whatever the map."""
    lo, hi = np.asarray(lo, U16), np.asarray(hi, U16)
    nan = (lo == 0x7FC0) | (hi == 0x7FC0)
    l, h = np.where(nan, 0, lo).astype(np.int64), np.where(nan, 0, hi).astype(np.int64)
    assert l.max(initial=0) <= 0x7F80 and h.max(initial=0) <= 0x7F80 and np.all(l <= h), "a probability's interval left [0, +inf]"
    key = bf16_order(table).astype(np.int64)
    out_lo, out_hi = table[l], table[h]
    und = np.nonzero((l != h).reshape(-1))[0]
    if und.size:
        lu, hu = l.reshape(-1)[und], h.reshape(-1)[und]
        imin, imax = lu.copy(), lu.copy()
        for step in range(1, int((hu - lu).max()) + 1):
            i = np.minimum(lu + step, hu)
            imin = np.where(key[i] < key[imin], i, imin)
            imax = np.where(key[i] > key[imax], i, imax)
        out_lo.reshape(-1)[und], out_hi.reshape(-1)[und] = table[imin], table[imax]
    return np.where(nan, U16(0x7FC0), out_lo).astype(U16), np.where(nan, U16(0x7FC0), out_hi).astype(U16)


def _row_granules(grid_bits, plo, phi):
    """Per row of admissible probabilities [plo, phi] (float64 values on the grid `grid_bits` of fq_P): a weight that every non-zero
    admissible P' of the row is an integer multiple of.  Grids are finer near zero, so it is the smallest lowest-bit weight (_lowbit)
    among the grid's values FROM the row's smallest non-zero admissible value UP; an element that may be zero or not (plo = 0 < phi)
    admits every grid value below phi, so it counts with the grid's smallest non-zero value.  A row without a non-zero value: inf."""
    grid = np.unique(_b64(grid_bits))
    grid = grid[np.isfinite(grid) & (grid > 0)]
    from_here_up = np.minimum.accumulate(_lowbit(grid)[::-1])[::-1]
    smallest = np.where(plo > 0, plo, np.where(phi > 0, grid[0], np.inf)).min(axis=-1)
    idx = np.minimum(np.searchsorted(grid, smallest), len(grid) - 1)
    return np.where(np.isfinite(smallest), from_here_up[idx], np.inf)


def attention_interval(q_bits, k_bits, v_bits, mask_bits, scaling, qmap, scale_bits=None, out_qmap=None, kernel="online"):
    """A whole attention core on bf16 patterns with the admissible interval of every output: q [B,H,Sq,D], k / v [B,H,Sk,D] (already
    fake-quantized), mask additive bf16 broadcastable to [B,H,Sq,Sk] or None, scaling a python float (multiplied as fp32), qmap / scale_bits
    the probabilities' fake-quantizer (None: none / unit scale; scale_bits: ONE bf16 pattern, what the kernels round *scale to),
    out_qmap the consumer's value map applied to the result (out_fq), kernel one of ATTENTION_KERNELS (attention_probs_interval).
    The chain, with its rounding points (modules/quantizable/modeling_bert.py:118-158):

        S = bf16(q k^T)            REQUIRED EXACT: q and k are small integers times a power of two, so every partial sum of the products,
                                   in any order, fits 24 bits (_sums_exact_in_f32); ValueError otherwise -- a case that breaks the premise
                                   fails here and does not loosen a check.  S is then bit-defined (one rounding of the exact sum),
        t = bf16(bf16(S x scaling) + mask)       bit-defined (scale_and_mask),
        p = bf16(softmax(t))       FIRST INEXACT ROUNDING: attention_probs_interval(t, kernel) -> [p_lo, p_hi],
        P' = fq_P(p)               a map of the pattern: the image of [p_lo, p_hi] (_image_of_interval; [fq(p_lo), fq(p_hi)] where monotone),
        O = bf16(sum_k P'_k v_k)   bounds: O_lo = sum_k (v_k >= 0 ? P'_lo : P'_hi) v_k, O_hi likewise with the ends swapped.

    The P'.V sum: P' lies on the grid of fq_P's values, v is a multiple of its own lowest bit; where the products' granule keeps the
    row's sum of absolute values within 24 bits the fp32 sum is exact in any order and the bounds above are final (asserted by the tests
    for e4m3, e5m2, posit8_1, fp4_e2m1 and int8 at a power-of-two scale); so are they where a sum has at most one non-zero term.
    Otherwise (no fq_P, posit8_2, other scales) the sum carries d_pv u sum |P'_hi v|, d_pv = max(SUM_DEPTH, ceil(Sk / 32) + 16): one
    accumulator rounding per 32-key matrix instruction (qt_attention.hip:400, qt_attention_rows.hip:322) and 16 for the additions inside
    one, the other key group's half included (qt_attention_rows.hip:337).  The granule of a row is _row_granules' (the grid's finest step from
    the row's smallest admissible P' up) times the lowest-bit weight of v.
    kernel = "strip_fp8" (qt_attention_fp8.hip) does NOT add in fp32: both products run on v_mfma_scale_f32_16x16x128_f8f6f4, which adds
    its 128 products in a tree of its own.  What that tree keeps when the products of one instruction span many binades -- the
    probabilities' do: 2^-18 .. 2 on the e5m2 grid -- is not documented, so no radius can be DERIVED for a P'.V sum of several terms
    (:335) and this kernel is pinned only where a sum has at most ONE non-zero term (v holds one key per column: exact whatever the
    tree does); ValueError otherwise.  For the scores (:114) the premise is exactness as above: their products are multiples of 2^-4
    spanning at most 2^6, the sum at most 2^12 granules; the GPU test's P' comparison then holds the tree to that, to the bit.
    Then ONE rounding to bf16 (_bf16_of) and, with out_qmap, the consumer's map (monotone).
    Rows: a NaN row of P stays NaN in every output element (NaN x 0 = NaN); fully masked rows as in attention_probs_interval.
    The observer's amax is max P in front of fq_P: [max p_lo, max p_hi], NaN if any row is.
    Returns AttentionIntervals."""
    q, k, v = _b64(q_bits), _b64(k_bits), _b64(v_bits)
    with np.errstate(all="ignore"):
        qf, kf = np.where(np.isfinite(q), q, 0.0), np.where(np.isfinite(k), k, 0.0)
        granule = _lowbit(qf).min() * _lowbit(kf).min()
        abs_s = np.einsum("bhqd,bhkd->bhqk", np.abs(qf), np.abs(kf))
        if not bool(np.all(_sums_exact_in_f32(abs_s, granule))):
            raise ValueError("attention_interval: the score sums are not exact in fp32 (q, k must be small integers times a power of two)")
        S = np.einsum("bhqd,bhkd->bhqk", q, k)
        # (np.einsum adds 0 x inf = NaN terms like the hardware; an fp64 sum of exactly representable partial sums is exact)
        s_bits = f32_to_bf16(S.astype(F32))
    t = scale_and_mask(s_bits, mask_bits, scaling)
    p = attention_probs_interval(t, kernel)
    table = _prob_fq(qmap, scale_bits)(np.arange(0x7F81, dtype=U32).astype(U16))      # fq_P of every non-negative bf16 pattern, +inf included
    grid_bits = table[:0x3F81]                                                        # ... of [0, 1]
    plo_bits, phi_bits = _image_of_interval(table, p.lo, p.hi)
    probs = RowInterval(p.v, p.rho, plo_bits, phi_bits)
    # amax
    nan_any = bool(p.nan.any())
    klo, khi = bf16_order(p.lo), bf16_order(p.hi)
    i_lo, i_hi = np.unravel_index(np.argmax(klo), klo.shape), np.unravel_index(np.argmax(khi), khi.shape)
    amax = RowInterval(np.array([np.nan if nan_any else np.nanmax(p.v)]), np.array([np.nan if nan_any else np.nanmax(p.rho)]),
                       np.array([0x7FC0 if nan_any else p.lo[i_lo]], U16), np.array([0x7FC0 if nan_any else p.hi[i_hi]], U16))
    # P'.V
    with np.errstate(all="ignore"):
        plo, phi = _b64(probs.lo), _b64(probs.hi)
        vp, vn = np.maximum(v, 0.0), np.minimum(v, 0.0)
        o_lo = plo @ vp + phi @ vn
        o_hi = phi @ vp + plo @ vn
        abs_o = phi @ np.abs(v)
        nnz = (phi > 0).astype(np.float64) @ (v != 0).astype(np.float64)
        granule_pv = (np.zeros(plo.shape[:-1]) if qmap is None else _row_granules(grid_bits, plo, phi)) * _lowbit(v).min()
        row_abs = np.where(np.isnan(abs_o), 0.0, abs_o).max(axis=-1)
        pv_exact = np.asarray(_sums_exact_in_f32(row_abs, granule_pv), bool) & (granule_pv > 0)
        d_pv = max(SUM_DEPTH, -(-k.shape[-2] // 32) + 16)
        if kernel == "strip_fp8":
            if np.any(nnz > 1):
                raise ValueError("attention_interval: kernel 'strip_fp8' takes a v with at most one non-zero key per column")
            pv_exact = np.ones_like(pv_exact)
        rho_o = np.where(pv_exact[..., None] | (nnz <= 1), 0.0, d_pv * U_F32 * abs_o)
        lo, hi = _bf16_of(o_lo - rho_o), _bf16_of(o_hi + rho_o)
    if out_qmap is not None:
        lo, hi = vmap_bf16(lo, out_qmap), vmap_bf16(hi, out_qmap)
    out = RowInterval((o_lo + o_hi) / 2, (o_hi - o_lo) / 2 + rho_o, lo, hi)
    return AttentionIntervals(out, probs, amax, pv_exact)
