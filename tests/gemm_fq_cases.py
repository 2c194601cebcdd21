"""Case tables and input builders for the fake-quant GEMM (csrc/qt_gemm.hip: qt_linear_fq_bf16, qt_bmm_fq_bf16), shared by
tests/test_gemm_fq_cases_cpu.py (what the cases guarantee, without a GPU) and tests/test_gpu_gemm_fq.py (the launches).  A plain module,
imported by name; it holds no tests and never touches the device.

launch_gemm compiles gemm_fq_kernel<BMODE, OBS_B, B_NN> 16 times; `instantiation` restates its rule, `UniformDiv` restates the divisor
record of csrc/qt_device.h in float32 numpy.  Operands travel as bf16 bit patterns (uint16), like everywhere in the oracle."""
import re

import numpy as np

from oracle import qt_oracle as o

F32, U32, U16 = np.float32, np.uint32, np.uint16

# ---- launch_gemm's rule -----------------------------------------------------------------------------------------------------------------
KIND_LUT, KIND_IDENTITY, KIND_FP_SAT, KIND_INT = 0, 1, 2, 3            # include/qt_hip.h: QT_FMT_*
B_PASS, B_FP_UNIT, B_FP_FAST, B_INT_FAST, B_GENERIC = 0, 1, 2, 3, 4    # csrc/qt_gemm.hip: kBPass ... kBGeneric
MODE_NAMES = {B_PASS: "kBPass", B_FP_UNIT: "kBFpUnit", B_FP_FAST: "kBFpFast", B_INT_FAST: "kBIntFast", B_GENERIC: "kBGeneric"}


def format_kind(dtype):
    """qt_format_for's kind of a dtype name: the closed forms (identity, e4m3 / e5m2, intN / uintN), a table for everything else."""
    if dtype is None:
        return KIND_IDENTITY
    if re.fullmatch(r"(?:fp8\.)?(e4m3|e5m2)", dtype):
        return KIND_FP_SAT
    if re.fullmatch(r"u?int(\d+)", dtype):
        return KIND_INT
    return KIND_LUT


def instantiation(kind, has_scale, has_obs, nn):
    """(format kind, scale pointer present, observer present, B n-contiguous) -> (BMODE, OBS_B, B_NN), as launch_gemm picks it."""
    if kind == KIND_IDENTITY and not has_scale and not has_obs:
        return (B_PASS, False, nn)
    if kind == KIND_FP_SAT and not has_scale:
        return (B_FP_UNIT, has_obs, nn)
    if kind == KIND_FP_SAT:
        return (B_FP_FAST, has_obs, nn)
    if kind == KIND_INT and has_scale:
        return (B_INT_FAST, has_obs, nn)
    return (B_GENERIC, False, nn)


ALL_INSTANTIATIONS = frozenset([(B_PASS, False, nn) for nn in (False, True)] + [(B_GENERIC, False, nn) for nn in (False, True)]
                               + [(m, obs, nn) for m in (B_FP_UNIT, B_FP_FAST, B_INT_FAST) for obs in (False, True) for nn in (False, True)])
assert len(ALL_INSTANTIATIONS) == 16


# ---- UniformDiv (csrc/qt_device.h) in float32 -------------------------------------------------------------------------------------------
def bf16_scale(scale):
    """The scale as the kernel uses it: the float32 behind the pointer rounded to bf16.  -> (float32 value, bf16 bits as uint16[1])"""
    bits = o.f32_to_bf16(np.array([scale], F32))
    return o.bf16_to_f32(bits)[0], bits


class UniformDiv:
    def __init__(self, scale):
        self.s = F32(scale)
        with np.errstate(all="ignore"):
            self.r = F32(1.0) / self.s
        a = int(np.array([self.s], F32).view(U32)[0]) & 0x7FFFFFFF
        self.safe = ((127 - 100) << 23) <= a <= ((127 + 100) << 23)
        self.pow2 = (a & 0x007FFFFF) == 0

    def fast16(self, x):
        """x * RN(1 / s) and fast16's flag: the low half of the product within 3 of the bf16 rounding's decision point."""
        with np.errstate(all="ignore"):
            q = (np.asarray(x, F32) * self.r).astype(F32)
        flag = (((q.view(U32) + U32(3) - U32(0x8000)) & U32(0xFFFF)) <= U32(6)) & (not self.pow2)
        return q, flag

    def exact(self, x):
        with np.errstate(all="ignore"):
            return (np.asarray(x, F32) / self.s).astype(F32)


# ---- scales -----------------------------------------------------------------------------------------------------------------------------
# Two non-power-of-two scales.  GENERAL is the kind a calibrated tensor has; fast16 flags nothing at it.  REDO is one at which fast16
# flags 86 of the 65 536 bf16 patterns, so quant_vec's redo with the full division runs (asserted in test_gemm_fq_cases_cpu.py, which
# also states why no scale makes the redo change a result on bf16 operands).
GENERAL_SCALE = 0.037109375          # bf16 0x3D18 (0.037 rounded)
REDO_SCALE = 6.0                     # bf16 0x40C0
UNSAFE_SCALES = (2.0 ** -110, 2.0 ** 110)          # bf16-exact, outside UniformDiv.safe: the kernels' run-time fallback to the generic path
SCALE_CLASSES = (1.0, 0.25, GENERAL_SCALE, REDO_SCALE) + UNSAFE_SCALES
NON_POW2_SCALES = (GENERAL_SCALE, REDO_SCALE)


class BMode:
    """One way of quantizing an operand: format, scale behind a pointer (None: no pointer), observer."""

    def __init__(self, dtype, scale, obs):
        self.dtype, self.scale, self.obs = dtype, scale, obs
        self.kind = format_kind(dtype)

    def inst(self, nn):
        return instantiation(self.kind, self.scale is not None, self.obs, nn)

    @property
    def id(self):
        s = "noscale" if self.scale is None else f"s{self.scale:.4g}"
        return f"{self.dtype or 'identity'}-{s}-{'obs' if self.obs else 'noobs'}"

    def qmap(self):
        return o.get_quantization_map(self.dtype)

    def scale_bits(self):
        return bf16_scale(1.0 if self.scale is None else self.scale)[1]

    def fq(self, bits):
        """The oracle's fake-quant of a bf16 tensor under this mode (bits in, bits out, NaN canonical)."""
        return o.canon_nan16(o.fq_bf16(bits, self.qmap(), self.scale_bits()))


def _tier1_b_modes():
    modes = [BMode(None, None, False)]                                                        # kBPass
    for obs in (False, True):
        modes += [BMode(d, None, obs) for d in ("e4m3", "e5m2")]                              # kBFpUnit
        modes += [BMode(d, s, obs) for d in ("e4m3", "e5m2") for s in SCALE_CLASSES]          # kBFpFast (+ the !safe fallback)
        modes += [BMode(d, s, obs) for d in ("int8", "uint8", "int4") for s in SCALE_CLASSES]  # kBIntFast (+ the !safe fallback)
        modes += [BMode("int8", None, obs), BMode("posit8_1", None, obs), BMode("posit8_1", GENERAL_SCALE, obs)]   # kBGeneric
    modes += [BMode(None, GENERAL_SCALE, False), BMode(None, GENERAL_SCALE, True), BMode(None, None, True)]        # kBGeneric: identity
    return modes


TIER1_B_MODES = _tier1_b_modes()
TIER1_A_MODES = [BMode(d, s, obs) for obs in (False, True)
                 for d, s in (("e4m3", None), ("e4m3", GENERAL_SCALE), ("int8", GENERAL_SCALE), ("posit8_1", None))]

# the entry points and layouts every Tier 1 B mode runs through: (entry point, B n-contiguous)
ROUTES = (("linear", False), ("bmm", False), ("bmm", True))


def reached(modes=None):
    """{entry point: set of instantiations} the Tier 1 table launches."""
    out = {"linear": set(), "bmm": set()}
    for m in (TIER1_B_MODES if modes is None else modes):
        for entry, nn in ROUTES:
            out[entry].add(m.inst(nn))
    return out


# ---- Tier 1: every bf16 pattern through the staged fake-quantizer -----------------------------------------------------------------------
SEL_ROWS, SEL_K = 512, 128            # 65 536 patterns as 512 x 128 against the 128 x 128 identity


def identity_bits(n=SEL_K):
    return o.f32_to_bf16(np.eye(n, dtype=F32))


def selector_operand(mode):
    """(W bits 512 x 128, expected fq(W) bits): all 65 536 patterns, +0 written where the oracle's quantized value is not finite (0 * Inf
    would pollute a whole output column)."""
    w = o.all_bf16_patterns().reshape(SEL_ROWS, SEL_K).copy()
    w[~np.isfinite(o.bf16_to_f32(mode.fq(w)))] = 0
    return w, mode.fq(w)


def pos_zero(bits):
    """-0 -> +0 (the accumulator starts at +0, so a selected -0 comes out as +0)."""
    b = np.array(bits, dtype=U16, copy=True)
    b[b == 0x8000] = 0
    return b


def is_subnormal(bits):
    b = np.asarray(bits, U16)
    return ((b & 0x7F80) == 0) & ((b & 0x007F) != 0)


# ---- Tier 2: operands whose products and sums are exact in fp32 -------------------------------------------------------------------------
EXACT_LINEAR_SHAPES = ((1, 8, 8), (127, 72, 56), (128, 128, 64), (129, 136, 72), (200, 130, 136), (130, 264, 200))
EXACT_MODES = {"int8": (BMode("int8", 2.0 ** -6, True), 2.0 ** -6),         # codes times 2^-6
               "e4m3": (BMode("e4m3", None, True), 2.0 ** -9)}              # |w| in [2^-6, 2): multiples of 2^-9
NN_SIZES = (8, 72, 136)


def exact_operands(shape, which, seed, batch=None):
    """A (integers in [-4, 4]), W (raw bf16 values the mode quantizes to multiples of the quantum), bias (a multiple of the quantum).
    shape (M, N, K); W is returned as (N, K) -- k contiguous -- per batch.  -> dict of bf16 bits plus 'quantum'."""
    M, N, K = shape
    lead = () if batch is None else (batch,)
    g = np.random.default_rng(seed)
    a = g.integers(-4, 5, size=lead + (M, K)).astype(F32)
    mode, quantum = EXACT_MODES[which]
    if which == "int8":
        w = (g.standard_normal(lead + (N, K)) * 0.9).astype(F32)            # |w| / 2^-6 reaches past 127: clamped codes included
    else:
        w = (np.exp2(g.uniform(-6.0, 1.0, size=lead + (N, K))) * g.choice([-1.0, 1.0], size=lead + (N, K))).astype(F32)
        w = np.clip(w, -1.9375, 1.9375)
        w = np.where(np.abs(w) < 2.0 ** -6, np.copysign(F32(2.0 ** -6), w), w).astype(F32)
    bias = (g.integers(-512, 513, size=(N,)) * quantum * 8).astype(F32)
    return {"a": o.f32_to_bf16(a), "w": o.f32_to_bf16(w), "bias": o.f32_to_bf16(bias), "quantum": quantum, "mode": mode}


def exact_product(a_bits, wq_bits, bias_bits=None):
    """fp64 A @ Wq^T (+ bias) over the last two axes and its single rounding to bf16.  wq_bits: the QUANTIZED weights, (.., N, K)."""
    a = o.bf16_to_f32(a_bits).astype(np.float64)
    w = o.bf16_to_f32(wq_bits).astype(np.float64)
    y = a @ np.swapaxes(w, -1, -2)
    if bias_bits is not None:
        y = y + o.bf16_to_f32(bias_bits).astype(np.float64)
    return y, o.f32_to_bf16(y.astype(F32))


def abs_sum_quanta(a_bits, wq_bits, bias_bits, quantum):
    """max over the outputs of (sum_k |a| |w| + |bias|) / quantum: below 2^24, every partial sum in any order is an fp32 integer multiple
    of the quantum, hence exact."""
    a = np.abs(o.bf16_to_f32(a_bits).astype(np.float64))
    w = np.abs(o.bf16_to_f32(wq_bits).astype(np.float64))
    y = a @ np.swapaxes(w, -1, -2)
    if bias_bits is not None:
        y = y + np.abs(o.bf16_to_f32(bias_bits).astype(np.float64))
    return float(y.max()) / quantum


def on_quantum(bits, quantum):
    v = o.bf16_to_f32(bits).astype(np.float64) / quantum
    return bool(np.all(v == np.rint(v)))


# ---- Tier 3: general scales, the project's tolerance ------------------------------------------------------------------------------------
TOL_MODES = (("e4m3", 0.037), ("int8", 0.0173), ("int4", 0.11))
TOL_LINEAR_SHAPES = ((100, 72, 136), (333, 130, 1000))
TOL_BMM_NN = (2, 100, 72, 136)                   # batch, M, N, K
SHARE = 1e-2


def tol_operands(shape, seed, batch=None):
    """x ~ N(0, 1), W ~ N(0, 0.05), bias ~ N(0, 1), as tests/test_gpu_parity.py::test_linear_fq_gemm draws them."""
    M, N, K = shape
    lead = () if batch is None else (batch,)
    g = np.random.default_rng(seed)
    return {"a": o.f32_to_bf16(g.standard_normal(lead + (M, K)).astype(F32)),
            "w": o.f32_to_bf16((g.standard_normal(lead + (N, K)) * 0.05).astype(F32)),
            "bias": o.f32_to_bf16(g.standard_normal(N).astype(F32))}


def products_close(got_bits, ref64):
    """tests/test_gpu_parity.py::_products_close on host arrays: every element within 2^-7 |ref| + 2^-16 max|ref| of the fp64 product, and
    at most SHARE of them different from that product rounded once.  -> (ok, bit-equal share, worst excess over the bound)"""
    ref_bits = o.f32_to_bf16(ref64.astype(F32))
    same = float(np.mean(np.asarray(got_bits, U16) == ref_bits))
    err = np.abs(o.bf16_to_f32(got_bits).astype(np.float64) - ref64)
    bound = 2.0 ** -7 * np.abs(ref64) + 2.0 ** -16 * float(np.abs(ref64).max())
    return same >= 1.0 - SHARE and bool((err <= bound).all()), same, float((err - bound).max())


def f32_accumulated(a_bits, wq_bits, bias_bits, reverse):
    """The product accumulated in float32 in 32-wide k steps (first to last, or last to first), bias added in float32, rounded once."""
    a, w = o.bf16_to_f32(a_bits), o.bf16_to_f32(wq_bits)
    K = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (w.shape[-2],), F32)
    steps = list(range(0, K, 32))
    for k0 in (reversed(steps) if reverse else steps):
        part = np.einsum("...mk,...nk->...mn", a[..., k0:k0 + 32].astype(np.float64), w[..., k0:k0 + 32].astype(np.float64)).astype(F32)
        acc = (acc + part).astype(F32)
    if bias_bits is not None:
        acc = (acc + o.bf16_to_f32(bias_bits)).astype(F32)
    return o.f32_to_bf16(acc)


# ---- non-finite weights -----------------------------------------------------------------------------------------------------------------
NONFINITE_SHAPE = (128, 128, 64)
NONFINITE_MODES = [BMode(None, None, False), BMode("e4m3", None, False), BMode("e4m3", GENERAL_SCALE, False), BMode("int8", GENERAL_SCALE, True),
                   BMode("posit8_1", None, False)]
