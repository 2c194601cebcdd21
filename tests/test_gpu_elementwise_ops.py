"""The elementwise launches of csrc/qt_model_ops.hip -- the rotary family, the SiLU * up family and GELU -- through the C ABI, against
the restatements of oracle/qt_oracle.py (rope: bit for bit; silu_mul, gelu: an interval) on the inputs of oracle/elementwise_cases.py.
What the oracle alone guarantees for these inputs is asserted without a GPU in tests/test_oracle_elementwise_cpu.py.

Everywhere: guard bands around every output buffer untouched, a second launch bit-identical to the first, NaN exactly where the oracle
has NaN, a refused call writes nothing.  Rotary outputs equal o.rope bit for bit; FP8 codes and quantized values are the single pass
(qt_fake_quant_bf16_fp8, pinned elsewhere) on the oracle's values, table formats o.vmap_bf16 of them.  SiLU * up and GELU lie inside
the oracle's interval; the fused variants equal the consumer's single pass on the plain kernel's own output, which on the decided
elements IS the decided value -- so a fused variant cannot hide behind the interval.

Which case is there for which path (the launch code: qt_rope_bf16, rope_fq_launch, qt_rope_map_bf16, rope_map_value_launch,
qt_silu_mul_*, qt_gelu_bf16; "clamp" = the cap on workgroups, 256 * 32 = 8192 for the vector kernels, 256 * 64 = 16 384 token workgroups):

  second trips of the grid-stride loops
    rope_kernel             (1, 3301, 32, 8, 128): 3301 * 40 * 16 = 2 112 640 vectors = 8252.5 workgroups' worth > 8192: a second trip for
                            the first 60.5 * 256 vectors, stride gridDim.x * 256, crossing from q (1 689 600 vectors) into k on the first trip.
    silu_mul_kernel, _fq8, _map   4100 x 4104: 2 103 300 vectors = 8216.02 * 256: second trip, ragged end, row stride != cols.
    gelu_kernel             n = 8 * (8192 * 256 + 773): second trip of 773 vectors (plain and codes).
    rope_fq_kernel          (1, 16 421, 16, 1, 128): nv_max = 256 -> tpb = 1, 16 421 tokens > 16 384 workgroups: 37 tokens on a second trip.
    rope_fq_value_kernel    (1, 16 512, 16, 1, 128): tpb = 1, rope_blocks = 16 384, 129 value workgroups behind them, gridDim.x = 16 513:
                            the second trip's stride is rope_blocks * tpb, not gridDim.x * tpb (128 tokens would be skipped).
    rope_map_value_kernel   the same shape with a table format, and with 512 weight workgroups in front (bid = blockIdx.x - wp.blocks).
  the closed-form output branch of rope_fq_token (y8 == NULL, no map): test_rope_fq_token_packing with codes = False.
  inner quantizers: qt_rope_fq_inner_value (the four non-CODES instantiations of rope_fq_value_kernel; q only / k only / both), inner_q /
    inner_k in {00, 10, 01, 11} of qt_rope_map_bf16 and qt_rope_map_value.
  fewer key heads: Hk < Hq in every value-job case, in two of the four small qt_rope_bf16 shapes, in five of the six packing shapes and in
    every past-the-clamp case; the value tensor is [B, Hk, S, D] by strides (the job is sized by Hk, the token job by max(Hq, Hk)).
  all six instantiations of rope_fq_value_kernel: <false, D, true> (e4m3 values, codes only), <false, D> (e4m3 values, inner),
    <true, D> (e5m2 values; codes only and inner), D = 64 and 128.
  token packing (tpb = 256 / nv_max tokens per workgroup, nv_max = Hq D / 8):
    nv_max   2 -> tpb 128, 385 and 511 tokens (= 1 and 127 mod 128);   24 -> tpb 10, tpb * nv = 240, 21 and 39 tokens (1 and 9 mod 10);
    96 -> tpb 2 (192 lanes busy), 9 tokens;   254 -> tpb 1, two idle lanes;   256 -> tpb 1;   320 -> tpb 1, a second trip of the lane loop
    for 64 vectors.  With Hk < Hq the k pass of a workgroup has nv_k < nv_q: its lane loop ends earlier and `lt` divides by another nv.
  data edges: the planted token (elementwise_cases.PLANTS: inf - inf, inf * 0, max + max, fp32-subnormal products kept, a finite
    sum beyond both FP8 maxima) is in every rotary case; all 65 536 patterns are x in (3, 77, 8, 2, 64) and every past-the-clamp case;
    SiLU gates -88.5 | -89 (expf finite | inf), +-0, +-inf, NaN, the largest finite; ups into the FP8 saturation range; exact zeros.

Wall time on one MI355X: 15 s for the 54 tests (3.8 s of it the first test's set-up: loading the library and the device), the slowest
test 1.7 s (test_rope_fq_past_the_clamp, 33.6 M elements; the other past-the-clamp tests 1.2 - 1.6 s), every other below 0.5 s.
With -s the module prints, per interval family, the smallest decided share of a launch (planted values included: at 8 elements the
launch IS the planted values) and the worst distance from the interval:
    [elementwise] gelu: smallest decided share 0.6667, worst distance from the interval 0
    [elementwise] silu_mul: smallest decided share 0.9963, worst distance from the interval 0
The rotary outputs, the codes and the table formats are compared for equality and have no such figure.

Run on the MI355X box:  python -m pytest tests/test_gpu_elementwise_ops.py -m gpu -q
"""
import ctypes

import numpy as np
import pytest

from oracle import elementwise_cases as ec
from oracle import qt_oracle as o

from kernel_launch import dev, fq8_single, inside, launch, nv, print_stats, refused, same, stream, table_format  # noqa: F401

pytestmark = pytest.mark.gpu

TABLE_FORMATS = ("posit8_2", "fp6_e3m2", "fp4_e2m1")
FP8 = ("e4m3", "e5m2")
U16, U8 = np.uint16, np.uint8


def teardown_module(module):
    print_stats("elementwise")


def bhsd(y):
    """[B, S, H, D] -> [B, H, S, D], contiguous: the order the fused rotary kernels write."""
    return np.ascontiguousarray(y.transpose(0, 2, 1, 3))


def not_nan(bits):
    return o.canon_nan16(bits) != 0x7FC0


class RopeIn:
    """A rotary case on the device: q | k | v as column slices of one buffer (row stride rs > (Hq + 2 Hk) D), the tables, the oracle's
    outputs computed once."""

    def __init__(self, c):
        self.c = c
        self.B, self.S, self.Hq, self.D = c["q"].shape
        self.Hk = c["k"].shape[2]
        buf, self.rs, cq, ck, cv = ec.qkv_rows(c)
        self.buf, self.cos, self.sin = dev(buf), dev(c["cos"]), dev(c["sin"])
        self.q, self.k, self.v = (self.buf.data_ptr() + 2 * col for col in (cq, ck, cv))
        self.dims = (self.B, self.S, self.Hq, self.Hk, self.D, self.rs, self.rs)
        self.vstrides = (self.S * self.rs, self.D, self.rs)      # v as [B, Hk, S, D]
        self.qshape, self.kshape = (self.B, self.Hq, self.S, self.D), (self.B, self.Hk, self.S, self.D)
        self._ref = {}

    def tables(self, rotate=True):
        return (self.cos.data_ptr(), self.sin.data_ptr()) if rotate else (None, None)

    def ref(self, name, rotate=True, inner=None, out=None):
        """o.rope of q or k in [B, H, S, D] order; inner / out: format names (None: none)."""
        key = (name, rotate, inner, out)
        if key not in self._ref:
            qmap = lambda d: None if d is None else o.get_quantization_map(d)  # noqa: E731
            c = self.c
            self._ref[key] = bhsd(o.rope(c[name], c["cos"] if rotate else None, c["sin"] if rotate else None, qmap(inner), qmap(out)))
        return self._ref[key]

    def v_bhsd(self):
        return bhsd(self.c["v"])


_CASES = {}


def rope_in(shape, value=False):
    key = (shape, value)
    if key not in _CASES:
        _CASES.clear()                                            # (one case on the device at a time)
        _CASES[key] = RopeIn(ec.rope_case(*shape, value=value))
    return _CASES[key]


def check_fp8(nv, got, got8, ref, dtype, what):
    """got / got8 (either may be None): the quantized values and codes of the single pass on the oracle's values `ref`."""
    vals, codes = fq8_single(nv, ref, dtype)
    same(vals, o.vmap_bf16(ref, o.get_quantization_map(dtype)), what + ": the single pass is not the oracle's value map")
    if got is not None:
        same(got, vals, what + " values")
    if got8 is not None:
        same(got8, codes, what + " codes", not_nan(ref))


# ---- qt_rope_bf16 -----------------------------------------------------------------------------------------------------------------------
def rope_plain(nv, r, what):
    B, S, Hq, Hk, D = r.dims[:5]
    got = launch(lambda g: nv.lib().qt_rope_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, *r.dims, stream()),
                 {"q": ((B, S, Hq, D), U16), "k": ((B, S, Hk, D), U16)}, what)
    for name in ("q", "k"):
        same(got[name], o.rope(r.c[name], r.c["cos"], r.c["sin"]), f"{what} {name}")


@pytest.mark.parametrize("shape", ec.ROPE_SHAPES + (ec.ROPE_PAST_CLAMP,))
def test_rope_plain(nv, shape):
    """qt_rope_bf16 == o.rope bit for bit: D = 16 (one vector per half), 48, 64, 128, Hk < Hq and Hk == Hq, one workgroup and several;
    the last shape is past the clamp."""
    rope_plain(nv, rope_in(shape), f"qt_rope_bf16 {shape}")


def test_rope_plain_refusals(nv):
    r = rope_in((2, 5, 3, 1, 16))
    B, S, Hq, Hk, D, rs, _ = r.dims
    specs = {"q": ((B, S, Hq, D), U16), "k": ((B, S, Hk, D), U16)}
    L = nv.lib()
    refused(lambda g: L.qt_rope_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, B, S, Hq, Hk, 24, rs, rs, stream()), specs, "D % 16")
    refused(lambda g: L.qt_rope_bf16(r.q + 2, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, *r.dims, stream()), specs, "misaligned q")
    refused(lambda g: L.qt_rope_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr + 8, *r.dims, stream()), specs, "misaligned k_out")
    refused(lambda g: L.qt_rope_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, B, S, Hq, Hk, D, Hq * D - 8, rs, stream()), specs, "q row stride < Hq D")
    refused(lambda g: L.qt_rope_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, B, S, Hq, Hk, D, rs, Hk * D - 8, stream()), specs, "k row stride < Hk D")


# ---- qt_rope_fq_bf16 --------------------------------------------------------------------------------------------------------------------
def rope_fq(nv, r, dq, dk, codes, what):
    fq, fk = nv.format_for(dq), nv.format_for(dk)
    specs = {"q": (r.qshape, U16), "k": (r.kshape, U16)}
    if codes:
        specs.update({"q8": (r.qshape, U8), "k8": (r.kshape, U8)})
    got = launch(lambda g: nv.lib().qt_rope_fq_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, g["q8"].ptr if codes else None,
                                                    g["k8"].ptr if codes else None, *r.dims, ctypes.byref(fq), ctypes.byref(fk), stream()), specs, what)
    for name, d in (("q", dq), ("k", dk)):
        check_fp8(nv, got[name], got.get(name + "8"), r.ref(name), d, f"{what} {name}")


PACKING = [(Hq, Hk, D, T) for Hq, Hk, D, counts in ec.ROPE_FQ_PACKING for T in counts]


@pytest.mark.parametrize("Hq,Hk,D,T", PACKING)
def test_rope_fq_token_packing(nv, Hq, Hk, D, T):
    """qt_rope_fq_bf16 at every tokens-per-workgroup regime (module docstring), formats (e4m3, e5m2) and (e5m2, e4m3), with codes (the
    hardware conversion) and with q_out8 = k_out8 = NULL (the closed-form branch)."""
    B, S = ec.tokens_as(T)
    r = rope_in((B, S, Hq, Hk, D))
    for dq, dk in (FP8, FP8[::-1]):
        for codes in (True, False):
            rope_fq(nv, r, dq, dk, codes, f"qt_rope_fq_bf16 {(B, S, Hq, Hk, D)} {dq}/{dk} codes={codes}")


def test_rope_fq_past_the_clamp(nv):
    r = rope_in(ec.ROPE_FQ_PAST_CLAMP)
    assert r.c["patterns"]
    rope_fq(nv, r, "e4m3", "e5m2", True, f"qt_rope_fq_bf16 {ec.ROPE_FQ_PAST_CLAMP}")


def test_rope_fq_refusals(nv):
    r = rope_in((2, 5, 3, 1, 16))
    L = nv.lib()
    f = nv.format_for("e4m3")
    i8 = nv.format_for("int8")
    specs = {"q": (r.qshape, U16), "k": (r.kshape, U16), "q8": (r.qshape, U8), "k8": (r.kshape, U8)}
    fmts = (ctypes.byref(f), ctypes.byref(f), stream())
    refused(lambda g: L.qt_rope_fq_bf16(r.q, r.k, None, None, g["q"].ptr, g["k"].ptr, g["q8"].ptr, g["k8"].ptr, *r.dims, *fmts), specs, "values without tables")
    refused(lambda g: L.qt_rope_fq_bf16(r.q, r.k, *r.tables(), g["q"].ptr, None, g["q8"].ptr, g["k8"].ptr, *r.dims, *fmts), specs, "k_out missing")
    refused(lambda g: L.qt_rope_fq_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, g["q8"].ptr, g["k8"].ptr, *r.dims, ctypes.byref(i8), ctypes.byref(f), stream()),
            specs, "a format that is not FP")
    refused(lambda g: L.qt_rope_fq_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, g["q8"].ptr + 4, g["k8"].ptr, *r.dims, *fmts), specs, "misaligned codes")


# ---- qt_rope_fq_value, qt_rope_fq_inner_value -------------------------------------------------------------------------------------------
def value_codes_t(nv, v_bhsd, dtype):
    """(vt8 [B, Hk, D, S], mask of the comparable bytes): the single pass's codes of v, transposed, the keys of every 128-block in the
    k-slot order of csrc/qt_value_codes.h: slot 16 g + 4 t + e of each half of 64 holds key 16 t + 4 g + e."""
    B, H, S, D = v_bhsd.shape
    _, codes = fq8_single(nv, v_bhsd, dtype)
    pos = np.arange(128)
    key_of = (pos & 64) | (((pos >> 2) & 3) << 4) | (((pos >> 4) & 3) << 2) | (pos & 3)

    def t(a):
        return np.ascontiguousarray(a.reshape(B, H, S // 128, 128, D)[:, :, :, key_of, :].transpose(0, 1, 4, 2, 3)).reshape(B, H, D, S)
    return t(codes), t(not_nan(v_bhsd))


def rope_fq_value(nv, r, dq, dk, dv, inner, values, rotate, what):
    """inner: None (qt_rope_fq_value) or (format name or None for q, for k) (qt_rope_fq_inner_value)."""
    L = nv.lib()
    fq, fk, fv = nv.format_for(dq), nv.format_for(dk), nv.format_for(dv)
    specs = {"q8": (r.qshape, U8), "k8": (r.kshape, U8), "vt8": ((r.B, r.Hk, r.D, r.S), U8)}
    if values:
        specs.update({"q": (r.qshape, U16), "k": (r.kshape, U16)})
    head = lambda g: (r.q, r.k, *r.tables(rotate), g["q"].ptr if values else None, g["k"].ptr if values else None, g["q8"].ptr, g["k8"].ptr, *r.dims,  # noqa: E731
                      ctypes.byref(fq), ctypes.byref(fk))
    tail = lambda g: (r.v, g["vt8"].ptr, *r.vstrides, ctypes.byref(fv), stream())  # noqa: E731
    if inner is None:
        got = launch(lambda g: L.qt_rope_fq_value(*head(g), *tail(g)), specs, what)
    else:
        fi = [nv.format_for(d) if d is not None else None for d in inner]
        ip = [ctypes.byref(f) if f is not None else None for f in fi]
        got = launch(lambda g: L.qt_rope_fq_inner_value(*head(g), *ip, *tail(g)), specs, what)
    for i, (name, d) in enumerate((("q", dq), ("k", dk))):
        ref = r.ref(name, rotate, inner[i] if inner is not None else None)
        check_fp8(nv, got.get(name), got[name + "8"], ref, d, f"{what} {name}")
    want, ok = value_codes_t(nv, r.v_bhsd(), dv)
    same(got["vt8"], want, what + " vt8", ok)


@pytest.mark.parametrize("D,S", [(64, 128), (128, 384)])
@pytest.mark.parametrize("dv", FP8)
@pytest.mark.parametrize("mode", ["codes", "inner"])
def test_rope_fq_value_every_instantiation(nv, D, S, dv, mode):
    """All six instantiations of rope_fq_value_kernel (module docstring), Hq = 4 > Hk = 2, B = 2, the value tensor [B, Hk, S, D] by
    strides; q_out / k_out given and NULL; codes only also without a rotation (cos = sin = NULL, BERT's path); the inner quantizer on q
    only, on k only and on both (other formats than the outputs')."""
    shape = (2, S, 4, 2, D)
    r = rope_in(shape, value=True)
    for values in (True, False):
        if mode == "codes":
            for rotate in (True, False):
                rope_fq_value(nv, r, "e4m3", "e5m2", dv, None, values, rotate, f"qt_rope_fq_value {shape} v={dv} values={values} rotate={rotate}")
        else:
            for inner in (("e5m2", "e4m3"), ("e5m2", None), (None, "e5m2")):
                rope_fq_value(nv, r, "e4m3", "e5m2", dv, inner, values, True, f"qt_rope_fq_inner_value {shape} v={dv} values={values} inner={inner}")


def test_rope_fq_value_past_the_token_clamp(nv):
    shape = ec.ROPE_VALUE_PAST_CLAMP
    rope_fq_value(nv, rope_in(shape, value=True), "e4m3", "e4m3", "e4m3", None, False, True, f"qt_rope_fq_value {shape}")


def test_rope_fq_value_refusals(nv):
    L = nv.lib()
    f, i8 = nv.format_for("e4m3"), nv.format_for("int8")
    F = ctypes.byref(f)

    def call(r, g, D=None, S=None, rotate=True, inner=None):
        dims = list(r.dims)
        dims[1], dims[4] = S or r.S, D or r.D
        args = (r.q, r.k, *r.tables(rotate), None, None, g["q8"].ptr, g["k8"].ptr, *dims, F, F)
        tail = (r.v, g["vt8"].ptr, *r.vstrides, F, stream())
        return L.qt_rope_fq_value(*args, *tail) if inner is None else L.qt_rope_fq_inner_value(*args, *inner, *tail)
    r = rope_in((2, 128, 4, 2, 64), value=True)
    specs = {"q8": (r.qshape, U8), "k8": (r.kshape, U8), "vt8": ((r.B, r.Hk, r.D, r.S), U8)}
    refused(lambda g: call(r, g, S=64), specs, "S % 128")
    refused(lambda g: call(r, g, D=32), specs, "D = 32")
    refused(lambda g: call(r, g, rotate=False, inner=(F, F)), specs, "an inner quantizer without a rotation")
    refused(lambda g: call(r, g, inner=(ctypes.byref(i8), None)), specs, "an inner quantizer that is not FP")


# ---- qt_rope_map_bf16, qt_rope_map_value, qt_rope_map_value_weight ----------------------------------------------------------------------
def value_t_rows(v_bhsd, dtype):
    """vt [B, Hk, D, S]: the value map of v, transposed, the keys of every 32-chunk in the k-slot order of csrc/qt_value_rows.h:
    key 32 c + 16 h + 4 g + e -> slot 32 c + 8 g + 4 h + e."""
    vq = o.canon_nan16(o.vmap_bf16(v_bhsd, o.get_quantization_map(dtype)))
    key = np.arange(v_bhsd.shape[2])
    slot = (key & ~31) | (((key >> 2) & 3) << 3) | (((key >> 4) & 1) << 2) | (key & 3)
    want = np.empty(vq.shape[:2] + (vq.shape[3], vq.shape[2]), U16)
    want[..., slot] = vq.transpose(0, 1, 3, 2)
    return want


INNER_MODES = ((0, 0), (1, 0), (0, 1), (1, 1))


def check_rope_map(r, got, dtype, iq, ik, what):
    for name, inner in (("q", iq), ("k", ik)):
        same(got[name], r.ref(name, True, dtype if inner else None, dtype), f"{what} {name}")


@pytest.mark.parametrize("dtype", TABLE_FORMATS)
@pytest.mark.parametrize("shape", [(3, 7, 3, 1, 64), (2, 33, 4, 2, 128), (1, 6, 20, 4, 128)])
def test_rope_map_inner_modes(nv, shape, dtype):
    """qt_rope_map_bf16 == the value map of o.rope (the inner form where asked), both row-table sizes, tpb = 10 | 4 | 1."""
    r = rope_in(shape)
    fmt, lut = table_format(nv, dtype)
    for iq, ik in INNER_MODES:
        what = f"qt_rope_map_bf16 {shape} {dtype} inner={iq}{ik}"
        got = launch(lambda g: nv.lib().qt_rope_map_bf16(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, *r.dims, ctypes.byref(fmt), lut.data_ptr(), iq, ik,
                                                         stream()), {"q": (r.qshape, U16), "k": (r.kshape, U16)}, what)
        check_rope_map(r, got, dtype, iq, ik, what)


def rope_map_value(nv, r, dtype, iq, ik, w_elems, what):
    L = nv.lib()
    fmt, lut = table_format(nv, dtype)
    specs = {"q": (r.qshape, U16), "k": (r.kshape, U16), "vt": ((r.B, r.Hk, r.D, r.S), U16)}
    head = lambda g: (r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, *r.dims, ctypes.byref(fmt), lut.data_ptr(), iq, ik, r.v, g["vt"].ptr, *r.vstrides)  # noqa: E731
    if w_elems is None:
        got = launch(lambda g: L.qt_rope_map_value(*head(g), stream()), specs, what)
    else:
        wb = ec.weight_case(w_elems)
        w = dev(wb)
        specs["wq"] = ((w_elems,), U16)
        got = launch(lambda g: L.qt_rope_map_value_weight(*head(g), w.data_ptr(), g["wq"].ptr, w_elems, stream()), specs, what)
        same(got["wq"], o.vmap_bf16(wb, o.get_quantization_map(dtype)), what + " fq(W)")
    check_rope_map(r, got, dtype, iq, ik, what)
    same(got["vt"], value_t_rows(r.v_bhsd(), dtype), what + " vt")


W_SMALL, W_TAIL, W_SECOND_TRIP = 8, 8 * (256 * 4 * 3 + 5), 8 * (512 * 256 * 4 + 256 * 4 * 3 + 5)


@pytest.mark.parametrize("dtype", TABLE_FORMATS)
def test_rope_map_value_inner_modes_and_weight_job(nv, dtype):
    """qt_rope_map_value at every inner mode, Hq = 4 > Hk = 2 (the value job is sized by Hk: 2 * 2 * 4 workgroups of 64 keys), and
    qt_rope_map_value_weight with a weight of one vector (one workgroup, one lane), of 3077 vectors (4 workgroups: three full trips'
    worth of four vectors per lane and a tail of five) and of 512 * 1024 + 3077 vectors (the cap of 512 workgroups and a second trip)."""
    shape = (2, 256, 4, 2, 128)
    r = rope_in(shape, value=True)
    for iq, ik in INNER_MODES:
        rope_map_value(nv, r, dtype, iq, ik, None, f"qt_rope_map_value {shape} {dtype} inner={iq}{ik}")
    for w_elems, (iq, ik) in ((W_SMALL, (0, 0)), (W_TAIL, (1, 0)), (W_SECOND_TRIP, (0, 1))):
        rope_map_value(nv, r, dtype, iq, ik, w_elems, f"qt_rope_map_value_weight {shape} {dtype} w={w_elems}")


@pytest.mark.parametrize("w_elems", [None, W_SECOND_TRIP])
def test_rope_map_value_past_the_token_clamp(nv, w_elems):
    shape = ec.ROPE_VALUE_PAST_CLAMP
    rope_map_value(nv, rope_in(shape, value=True), "posit8_2", 1, 0, w_elems, f"qt_rope_map_value(_weight) {shape} w={w_elems}")


def test_rope_map_value_refusals(nv):
    L = nv.lib()
    r = rope_in((2, 128, 4, 2, 128), value=True)
    fmt, lut = table_format(nv, "posit8_2")
    plain = nv.format_for("posit8_2")
    specs = {"q": (r.qshape, U16), "k": (r.kshape, U16), "vt": ((r.B, r.Hk, r.D, r.S), U16)}

    def call(g, S=None, D=None, f=fmt, v=None):
        dims = list(r.dims)
        dims[1], dims[4] = S or r.S, D or r.D
        return L.qt_rope_map_value(r.q, r.k, *r.tables(), g["q"].ptr, g["k"].ptr, *dims, ctypes.byref(f), lut.data_ptr(), 0, 0, v or r.v, g["vt"].ptr, *r.vstrides,
                                   stream())
    refused(lambda g: call(g, S=64), specs, "S % 128")
    refused(lambda g: call(g, D=64), specs, "D = 64")
    refused(lambda g: call(g, f=plain), specs, "a table format not in its row form")
    refused(lambda g: call(g, v=r.v + 2), specs, "misaligned v")


# ---- SiLU * up --------------------------------------------------------------------------------------------------------------------------
def silu_all(nv, shape, fp8, tables):
    L = nv.lib()
    rows, cols = shape
    c = ec.silu_case(rows, cols)
    rs_g, rs_u = cols + 8, cols + 24
    g_dev, u_dev = dev(ec.strided(c["gate"], rs_g)), dev(ec.strided(c["up"], rs_u))
    gp, up = g_dev.data_ptr(), u_dev.data_ptr()
    what = f"qt_silu_mul_bf16 {rows}x{cols}"
    y = launch(lambda g: L.qt_silu_mul_bf16(gp, up, g["y"].ptr, rows, cols, rs_g, rs_u, stream()), {"y": (shape, U16)}, what)["y"]
    inside(o.silu_mul(c["gate"], c["up"]), y, what, "silu_mul")
    fin = not_nan(y)
    for d in fp8:
        fmt = nv.format_for(d)
        what = f"qt_silu_mul_fq8_bf16 {d} {rows}x{cols}"
        got = launch(lambda g: L.qt_silu_mul_fq8_bf16(gp, up, g["y"].ptr, g["y8"].ptr, rows, cols, rs_g, rs_u, ctypes.byref(fmt), stream()),
                     {"y": (shape, U16), "y8": (shape, U8)}, what)
        vals, codes = fq8_single(nv, y, d)
        same(got["y"], vals, what + " values")
        same(got["y8"], codes, what + " codes", fin)
    for d in tables:
        fmt, lut = table_format(nv, d)
        what = f"qt_silu_mul_map_bf16 {d} {rows}x{cols}"
        got = launch(lambda g: L.qt_silu_mul_map_bf16(gp, up, g["y"].ptr, rows, cols, rs_g, rs_u, ctypes.byref(fmt), lut.data_ptr(), stream()), {"y": (shape, U16)}, what)
        same(got["y"], o.vmap_bf16(y, o.get_quantization_map(d)), what)
    return c


@pytest.mark.parametrize("shape", ec.SILU_SHAPES)
def test_silu_mul_family(nv, shape):
    """qt_silu_mul_bf16 inside o.silu_mul's interval; _fq8_bf16 (e4m3, e5m2) and _map_bf16 (three table formats) the consumer's single
    pass / value map of the plain kernel's own output.  One vector; three long rows; 257 short ragged rows (row / col from the vector
    index with cols / 8 = 3); 5 x 4096.  gate and up row strides differ, both > cols."""
    silu_all(nv, shape, FP8, TABLE_FORMATS)


def test_silu_mul_past_the_clamp(nv):
    c = silu_all(nv, ec.SILU_PAST_CLAMP, ("e4m3",), ("posit8_2",))
    assert c["patterns"]


def test_silu_mul_refusals(nv):
    L = nv.lib()
    z = dev(np.zeros((4, 64), U16))
    p = z.data_ptr()
    f = nv.format_for("e4m3")
    fmt, lut = table_format(nv, "posit8_2")
    for cols, rs_g, rs_u, why in ((32, 24, 64, "gate stride < cols"), (32, 64, 24, "up stride < cols"), (28, 64, 64, "cols % 8")):
        specs = {"y": ((4, cols), U16), "y8": ((4, cols), U8)}
        refused(lambda g: L.qt_silu_mul_bf16(p, p, g["y"].ptr, 4, cols, rs_g, rs_u, stream()), specs, "qt_silu_mul_bf16: " + why)
        refused(lambda g: L.qt_silu_mul_fq8_bf16(p, p, g["y"].ptr, g["y8"].ptr, 4, cols, rs_g, rs_u, ctypes.byref(f), stream()), specs, "qt_silu_mul_fq8_bf16: " + why)
        refused(lambda g: L.qt_silu_mul_map_bf16(p, p, g["y"].ptr, 4, cols, rs_g, rs_u, ctypes.byref(fmt), lut.data_ptr(), stream()), specs, "qt_silu_mul_map_bf16: " + why)


# ---- GELU -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.GELU_SIZES + (ec.GELU_PAST_CLAMP,))
def test_gelu(nv, n):
    """qt_gelu_bf16 inside o.gelu's interval; with a consumer's FP8 format y and y8 are the single pass on the plain kernel's own output;
    y = NULL (codes only) writes the same codes.  One vector, 257 vectors (two workgroups), and past the clamp."""
    L = nv.lib()
    c = ec.gelu_case(n)
    x = dev(c["x"])
    what = f"qt_gelu_bf16 {n}"
    y = launch(lambda g: L.qt_gelu_bf16(x.data_ptr(), g["y"].ptr, None, n, None, stream()), {"y": ((n,), U16)}, what)["y"]
    inside(o.gelu(c["x"]), y, what, "gelu")
    assert c["patterns"] == (n == ec.GELU_PAST_CLAMP)
    fin = not_nan(y)
    for d in FP8 if n != ec.GELU_PAST_CLAMP else FP8[:1]:
        fmt = nv.format_for(d)
        vals, codes = fq8_single(nv, y, d)
        got = launch(lambda g: L.qt_gelu_bf16(x.data_ptr(), g["y"].ptr, g["y8"].ptr, n, ctypes.byref(fmt), stream()), {"y": ((n,), U16), "y8": ((n,), U8)},
                     f"{what} {d}")
        same(got["y"], vals, f"{what} {d} values")
        same(got["y8"], codes, f"{what} {d} codes", fin)
        only = launch(lambda g: L.qt_gelu_bf16(x.data_ptr(), None, g["y8"].ptr, n, ctypes.byref(fmt), stream()), {"y8": ((n,), U8)}, f"{what} {d} codes only")
        assert np.array_equal(only["y8"], got["y8"]), f"{what} {d}: the codes-only launch writes other codes"


def test_gelu_refusals(nv):
    L = nv.lib()
    x = dev(np.zeros(64, U16))
    f, i8 = nv.format_for("e4m3"), nv.format_for("int8")
    specs = {"y": ((64,), U16), "y8": ((64,), U8)}
    refused(lambda g: L.qt_gelu_bf16(x.data_ptr(), g["y"].ptr, g["y8"].ptr, 60, ctypes.byref(f), stream()), specs, "n % 8")
    refused(lambda g: L.qt_gelu_bf16(x.data_ptr(), g["y"].ptr, g["y8"].ptr, 64, ctypes.byref(i8), stream()), specs, "y8 with a format that is not FP8")
    refused(lambda g: L.qt_gelu_bf16(x.data_ptr(), g["y"].ptr, g["y8"].ptr, 64, None, stream()), specs, "y8 without a format")
    refused(lambda g: L.qt_gelu_bf16(x.data_ptr(), None, None, 64, None, stream()), specs, "no output")
