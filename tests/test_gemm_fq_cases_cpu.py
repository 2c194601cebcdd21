"""What tests/test_gpu_gemm_fq.py relies on, shown without a GPU (cases: tests/gemm_fq_cases.py).

(1) The Tier 1 table reaches all 16 instantiations of gemm_fq_kernel through the entry points that can reach them, plus the run-time
    fallback for scales outside the fast-division range, the redo branch, the generic kinds and the A-side kinds.
(2) What the fast division can and cannot do on bf16 operands (see test_redo_*).
(3) The exact-tier inputs are exact: sum |products| stays below 2^24 quanta, so fp32 accumulation in any order is the fp64 product.
(4) The tolerance-tier inputs leave room: an fp32 accumulation alone, in two orders, stays inside the project's product criterion.
"""
import numpy as np
import pytest

import gemm_fq_cases as gc
from oracle import qt_oracle as o

PATTERNS = o.all_bf16_patterns()
VALUES = o.bf16_to_f32(PATTERNS)


# ---- (1) coverage -----------------------------------------------------------------------------------------------------------------------
def test_instantiation_rule_on_its_corners():
    f = gc.instantiation
    assert f(gc.KIND_IDENTITY, False, False, False) == (gc.B_PASS, False, False)
    assert f(gc.KIND_IDENTITY, False, True, True) == (gc.B_GENERIC, False, True)           # observer only
    assert f(gc.KIND_IDENTITY, True, False, False) == (gc.B_GENERIC, False, False)         # identity with a scale
    assert f(gc.KIND_FP_SAT, False, True, True) == (gc.B_FP_UNIT, True, True)
    assert f(gc.KIND_FP_SAT, True, False, False) == (gc.B_FP_FAST, False, False)
    assert f(gc.KIND_INT, True, True, False) == (gc.B_INT_FAST, True, False)
    assert f(gc.KIND_INT, False, True, False) == (gc.B_GENERIC, False, False)              # an integer format without a scale
    assert f(gc.KIND_LUT, True, True, True) == (gc.B_GENERIC, False, True)
    assert [gc.format_kind(d) for d in (None, "e4m3", "e5m2", "int8", "uint8", "int4", "posit8_1", "fp8_e4m3")] == \
        [gc.KIND_IDENTITY, gc.KIND_FP_SAT, gc.KIND_FP_SAT, gc.KIND_INT, gc.KIND_INT, gc.KIND_INT, gc.KIND_LUT, gc.KIND_LUT]


def test_table_reaches_all_sixteen_instantiations():
    r = gc.reached()
    nt = {i for i in gc.ALL_INSTANTIATIONS if not i[2]}
    assert len(nt) == 8 and r["linear"] == nt, sorted(nt - r["linear"])                    # qt_linear_fq_bf16: the 8 NT ones
    assert r["bmm"] == set(gc.ALL_INSTANTIATIONS), sorted(set(gc.ALL_INSTANTIATIONS) - r["bmm"])
    assert len(r["linear"] | r["bmm"]) == 16


def test_table_reaches_the_paths_behind_the_instantiations():
    modes = gc.TIER1_B_MODES
    for inline in (gc.B_FP_FAST, gc.B_INT_FAST):
        for obs in (False, True):
            of = [m for m in modes if m.inst(False)[:2] == (inline, obs)]
            scales = {m.scale for m in of}
            assert set(gc.SCALE_CLASSES) <= scales, (gc.MODE_NAMES[inline], obs)
            assert any(not gc.UniformDiv(gc.bf16_scale(s)[0]).safe for s in scales)                       # the !dv.safe fallback
            assert any(gc.UniformDiv(gc.bf16_scale(s)[0]).fast16(VALUES)[1].any() for s in scales)        # the redo branch
    generic = {(m.kind, m.scale is not None, m.obs) for m in modes if m.inst(False)[0] == gc.B_GENERIC}
    assert {(gc.KIND_INT, False, False), (gc.KIND_INT, False, True)} <= generic                           # QT_FMT_INT without a scale
    assert {(gc.KIND_IDENTITY, True, False), (gc.KIND_IDENTITY, True, True)} <= generic                   # identity with a scale
    assert (gc.KIND_IDENTITY, False, True) in generic                                                     # identity, observer only
    assert {(gc.KIND_LUT, False, False), (gc.KIND_LUT, True, True)} <= generic                            # table, with and without a scale
    a_side = {(m.kind, m.scale is not None, m.obs) for m in gc.TIER1_A_MODES}
    for obs in (False, True):
        assert {(gc.KIND_FP_SAT, False, obs), (gc.KIND_FP_SAT, True, obs), (gc.KIND_INT, True, obs), (gc.KIND_LUT, False, obs)} <= a_side
    assert len({m.id for m in modes}) == len(modes) and len({m.id for m in gc.TIER1_A_MODES}) == len(gc.TIER1_A_MODES)


# ---- (2) the divisor record -------------------------------------------------------------------------------------------------------------
def test_scale_classes():
    for s in gc.SCALE_CLASSES:
        assert gc.bf16_scale(s)[0] == np.float32(s), s                                     # bf16-exact: the kernel's rounding changes nothing
    for s in gc.UNSAFE_SCALES:
        assert not gc.UniformDiv(s).safe and gc.UniformDiv(s).pow2
    for s in (1.0, 0.25):
        d = gc.UniformDiv(s)
        assert d.safe and d.pow2 and not d.fast16(VALUES)[1].any()
    for s in gc.NON_POW2_SCALES:
        d = gc.UniformDiv(s)
        assert d.safe and not d.pow2
    assert gc.UniformDiv(2.0 ** -100).safe and gc.UniformDiv(2.0 ** 100).safe
    assert not gc.UniformDiv(np.float32(2.0 ** -100) * np.float32(1 - 2.0 ** -8)).safe and not gc.UniformDiv(2.0 ** 100 * 1.0078125).safe


def test_redo_scale_is_flagged():
    """At REDO_SCALE fast16 flags bf16 patterns (86 of them, all with an fp32-subnormal quotient), so Tier 1 runs quant_vec's redo;
    at GENERAL_SCALE it flags none, so Tier 1 also runs the fast path on its own."""
    q, flag = gc.UniformDiv(gc.REDO_SCALE).fast16(VALUES)
    assert int(flag.sum()) == 86 and bool(np.all(np.abs(q[flag]) < 2.0 ** -126))
    assert not gc.UniformDiv(gc.GENERAL_SCALE).fast16(VALUES)[1].any()


def _quotients(scale):
    d = gc.UniformDiv(scale)
    q, flag = d.fast16(VALUES)
    return o.f32_to_bf16(q), o.f32_to_bf16(d.exact(VALUES)), flag


@pytest.mark.parametrize("exponent", [-100, -37, -6, -1, 0, 2, 3, 9, 64, 99])
def test_redo_never_changes_a_bf16_quotient(exponent):
    """The redo exists for elements whose fast quotient x * RN(1/s) rounds to another bf16 than x / s.  With x AND s bf16 there is no such
    element, at any scale: a bf16 rounding tie is an odd 9-bit significand t, so x / s within 5 fp32 ULPs of it would need
    |x - s t| <= 2^-21 |x| with x of 8 significant bits and s t an odd number of more than 8 -- never equal, and then at least
    2^-17 |x| apart; where the quotient is an fp32 subnormal the flag does fire (test_redo_scale_is_flagged), and both quotients
    still round alike.  Here: all 127 non-power-of-two significands of ten binades of the safe range, on all 65 536 patterns (the
    whole safe range was scanned once, 25 527 scales, with the same outcome).  So a kernel WITHOUT the redo computes the same results
    on these operands: Tier 1 pins the fast path and runs the redo branch, but cannot tell whether the branch is needed."""
    for m in range(1, 128):
        s = o.bf16_to_f32(np.array([((127 + exponent) << 7) | m], np.uint16))[0]
        fast, exact, flag = _quotients(s)
        differ = o.canon_nan16(fast) != o.canon_nan16(exact)
        assert not differ.any(), (float(s), int(differ.sum()), int((differ & flag).sum()))


# ---- (3) the exact tier -----------------------------------------------------------------------------------------------------------------
def _exact_cases():
    for i, shape in enumerate(gc.EXACT_LINEAR_SHAPES):
        for which in gc.EXACT_MODES:
            yield shape, which, None, 100 + i
    for n in gc.NN_SIZES:
        for k in gc.NN_SIZES:
            yield (40, n, k), "int8", 3, 200 + n + k
    yield (130, 136, 72), "e4m3", 3, 300


@pytest.mark.parametrize("shape,which,batch,seed", list(_exact_cases()))
def test_exact_tier_is_exact(shape, which, batch, seed):
    c = gc.exact_operands(shape, which, seed, batch)
    wq = c["mode"].fq(c["w"])
    assert gc.on_quantum(wq, c["quantum"]) and gc.on_quantum(c["bias"], c["quantum"]) and gc.on_quantum(c["a"], 1.0)
    assert np.abs(o.bf16_to_f32(c["a"])).max() <= 4
    assert not np.array_equal(wq, c["w"])                                                   # the quantizer has work to do
    assert gc.abs_sum_quanta(c["a"], wq, c["bias"], c["quantum"]) < 2.0 ** 24
    ref64, ref_bits = gc.exact_product(c["a"], wq, c["bias"])
    for reverse in (False, True):                                                           # ... and an fp32 accumulation agrees, bit for bit
        assert np.array_equal(gc.f32_accumulated(c["a"], wq, c["bias"], reverse), ref_bits)


# ---- (4) the tolerance tier -------------------------------------------------------------------------------------------------------------
def _tol_cases():
    for shape in gc.TOL_LINEAR_SHAPES:
        for dtype, scale in gc.TOL_MODES:
            yield shape, None, dtype, scale
    b, m, n, k = gc.TOL_BMM_NN
    yield (m, n, k), b, "e4m3", 0.037


@pytest.mark.parametrize("shape,batch,dtype,scale", list(_tol_cases()))
def test_fp32_accumulation_alone_meets_the_tolerance_tier(shape, batch, dtype, scale):
    c = gc.tol_operands(shape, sum(shape), batch)
    wq = gc.BMode(dtype, scale, False).fq(c["w"])
    bias = c["bias"] if batch is None else None
    ref64, _ = gc.exact_product(c["a"], wq, bias)
    for reverse in (False, True):
        ok, same, excess = gc.products_close(gc.f32_accumulated(c["a"], wq, bias, reverse), ref64)
        print(f"[gemm_fq cpu] {shape} {dtype} reverse={reverse}: bit-equal share {same:.5f}, worst excess {excess:.3e}")
        assert ok, (same, excess)
