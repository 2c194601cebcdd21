"""The elementwise oracles (oracle/qt_oracle.py: rope, silu_mul, gelu) and the inputs built for them (oracle/elementwise_cases.py),
without a GPU.

(1) rope is pinned, bit for bit, to Hugging Face's apply_rotary_pos_emb on CPU bf16 tensors -- fewer key heads than query heads and the
    planted edge values (inf - inf, inf * 0, a sum that overflows, fp32-subnormal products, -0 / NaN / subnormals in the tables)
    included; its inner form to the same chain with a CPU fake-quantizer between the product and the sum (torch's saturated float8
    round trip for the FP8 formats, the oracle's pinned fake-quant at unit scale for a table format).
(2) torch's CPU silu(g) * up and GELU lie inside the intervals of silu_mul and gelu, on every case the GPU tests launch below their
    past-the-clamp sizes and on all 65 536 patterns.  (torch's CPU GELU on bf16 flushes x / 2 where it is an fp32 subnormal,
    |x| < 2^-125, and multiplies by 1 + erf before it halves, which overflows for |x| >= 2^127 (NaN at +inf); at those inputs the comparison is with
    the kernel's documented expression written out in fp32 torch ops.)
(3) The closed forms of the degenerate regimes: gate <= -89 gives +-0 (NaN against an infinite up), gate -88.5 does not; NaN and inf
    propagate as IEEE says.
(4) The decided shares are conditions: the well-conditioned regime of every case decides >= 99 % (SiLU * up) and >= 98 % (GELU) of its
    finite elements.
"""
import numpy as np
import pytest
import torch

from oracle import elementwise_cases as ec
from oracle import qt_oracle as o


def t_bf16(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def bits_of(t):
    return o.canon_nan16(t.contiguous().view(torch.int16).numpy().view(np.uint16))


def hf_rope(c, inner=None):
    """apply_rotary_pos_emb on the case (inner None), or its chain with inner['q'] / inner['k'] applied to x * cos."""
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb, rotate_half
    q, k = t_bf16(c["q"]).transpose(1, 2), t_bf16(c["k"]).transpose(1, 2)       # [B, H, S, D], as the model holds them
    cos, sin = t_bf16(c["cos"]), t_bf16(c["sin"])
    if inner is None:
        yq, yk = apply_rotary_pos_emb(q, k, cos, sin)
    else:
        ident = lambda t: t  # noqa: E731
        yq, yk = ((inner.get(n) or ident)(x * cos.unsqueeze(1)) + rotate_half(x) * sin.unsqueeze(1) for n, x in (("q", q), ("k", k)))
    return bits_of(yq.transpose(1, 2)), bits_of(yk.transpose(1, 2))


# ---- (1) rope ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.ROPE_SHAPES + ((1, 5, 127, 5, 16), (2, 128, 4, 2, 64)))
def test_rope_restates_apply_rotary_pos_emb_bit_for_bit(shape):
    c = ec.rope_case(*shape)
    want_q, want_k = hf_rope(c)
    for name, want in (("q", want_q), ("k", want_k)):
        got = o.rope(c[name], c["cos"], c["sin"])
        assert np.array_equal(got, want), f"{name} {shape}: {int((got != want).sum())} of {got.size} differ"
    assert np.array_equal(o.rope(c["q"], None, None), o.canon_nan16(c["q"]))    # no rotation


def test_rope_planted_edges_have_their_closed_forms():
    """The planted token of a case: what each edge must give, independent of torch."""
    B, S, Hq, Hk, D = 3, 77, 8, 2, 64
    c = ec.rope_case(B, S, Hq, Hk, D)
    assert c["patterns"]
    assert np.array_equal(np.sort(np.unique(c["q"])), o.all_bf16_patterns())    # every pattern appears as x
    for name in ("q", "k"):
        y = o.rope(c[name], c["cos"], c["sin"])[0, 1, 0]
        assert y[0] == ec.NAN and y[2] == ec.NAN and y[6] == ec.NAN               # inf - inf, inf * 0, NaN in the table
        assert y[1] == ec.POS_INF                                               # max + max
        assert y[3] == 0x0012                                                   # 2.25 * 2^-130 = 18 * 2^-133: kept, not flushed
        assert y[4] == 0x8012                                                   # bf16(2^-134) = 0 (tie to even) minus the same product
        assert y[5] == 0x4768                                                   # 3 * -0 + 59392
        for fmt, fmax in (("e4m3", 0x43E0), ("e5m2", 0x4760)):                  # behind the consumer: inf and NaN are NaN, 59392 saturates
            yq = o.rope(c[name], c["cos"], c["sin"], out_qmap=o.get_quantization_map(fmt))[0, 1, 0]
            assert list(yq[[1, 0, 5]]) == [ec.NAN, ec.NAN, fmax]


def _float8_round_trip(dtype, fmax):
    """The stateless FP8 fake-quantizer at unit scale as torch ops: saturate, round to the format, a zero result is +0, non-finite -> NaN."""
    def fq(t):
        r = t.clamp(-fmax, fmax).to(dtype).to(torch.bfloat16)
        r = torch.where(r == 0, torch.zeros_like(r), r)
        return torch.where(t.isfinite(), r, torch.full_like(t, float("nan")))
    return fq


@pytest.mark.parametrize("shape", [(2, 5, 3, 1, 16), (2, 33, 4, 4, 128)])
def test_rope_inner_form_restates_the_chain_with_a_fake_quantizer_on_the_product(shape):
    c = ec.rope_case(*shape)
    e4, e5 = _float8_round_trip(torch.float8_e4m3fn, 448.0), _float8_round_trip(torch.float8_e5m2, 57344.0)
    m4, m5 = o.get_quantization_map("e4m3"), o.get_quantization_map("e5m2")
    for inner, maps in (({"q": e5, "k": e4}, {"q": m5, "k": m4}), ({"q": e4}, {"q": m4, "k": None}), ({"k": e5}, {"q": None, "k": m5})):
        want = dict(zip(("q", "k"), hf_rope(c, inner)))
        for name in ("q", "k"):
            got = o.rope(c[name], c["cos"], c["sin"], inner_qmap=maps[name])
            assert np.array_equal(got, want[name]), f"{name} {shape} {sorted(inner)}: {int((got != want[name]).sum())} differ"
    # a table format: the oracle's pinned fake-quant at unit scale as the CPU fake-quantizer
    mp = o.get_quantization_map("posit8_2")
    table = lambda t: t_bf16(o.fq_bf16(bits_of(t), mp, np.uint16(ec.ONE)))  # noqa: E731
    want = dict(zip(("q", "k"), hf_rope(c, {"q": table, "k": table})))
    for name in ("q", "k"):
        got = o.rope(c[name], c["cos"], c["sin"], inner_qmap=mp, out_qmap=mp)
        assert np.array_equal(got, o.canon_nan16(o.vmap_bf16(want[name], mp))), f"{name} {shape} posit8_2"


# ---- (2) - (4) SiLU * up ----------------------------------------------------------------------------------------------------------------
def torch_silu_mul(g_bits, u_bits):
    return bits_of(torch.nn.functional.silu(t_bf16(g_bits)) * t_bf16(u_bits))


@pytest.mark.parametrize("shape", ec.SILU_SHAPES + ((64, 4096),))
def test_silu_mul_interval_holds_torch_and_decides_the_well_conditioned_regime(shape):
    c = ec.silu_case(*shape)
    iv = o.silu_mul(c["gate"], c["up"])
    got = torch_silu_mul(c["gate"], c["up"])
    assert int(iv.distance(got).max()) == 0, f"{shape}: {iv.report(got)}"
    assert c["patterns"] == (shape == (64, 4096))
    well = c["well"]
    if well.any():
        share = iv.rows(well).decided_share()
        assert share >= ec.SILU_SHARE, f"{shape}: {share:.4f} of the well-conditioned elements decided"
        assert bool(np.isfinite(iv.v[well]).all())


def test_silu_mul_all_patterns_and_degenerate_gates():
    allp = o.all_bf16_patterns()
    for up in (ec.ONE, ec.MINUS_ONE, 0x4768, ec.POS_INF):
        u = np.full(65536, up, np.uint16)
        iv = o.silu_mul(allp, u)
        got = torch_silu_mul(allp, u)
        assert int(iv.distance(got).max()) == 0, f"up {up:#x}: {iv.report(got)}"
    one = np.array([ec.ONE], np.uint16)

    def s(g, u=one):
        iv = o.silu_mul(np.array([g], np.uint16), u)
        return int(iv.lo[0]), int(iv.hi[0])
    for g in (0xC2B2, 0xC300, ec.NEG_MAX):                        # -89, -128, the most negative finite gate: expf overflows, the quotient is -0
        lo, hi = s(g)
        assert lo & 0x7FFF == 0 and hi & 0x7FFF == 0, hex(g)
        assert s(g, np.array([ec.POS_INF], np.uint16)) == (ec.NAN, ec.NAN)      # 0 * inf
    assert s(0xC2B1) == (0x82DD, 0x82DD)                          # -88.5: e^88.5 is finite, the quotient -3.3e-37 is a normal fp32 number
    assert s(ec.NEG_INF) == (ec.NAN, ec.NAN) and s(ec.NAN) == (ec.NAN, ec.NAN)  # -inf / inf
    assert s(ec.POS_INF) == (ec.POS_INF, ec.POS_INF) and s(ec.MAX) == (ec.MAX, ec.MAX)
    assert s(0x0000) == (0, 0) and s(ec.NEG_ZERO)[0] & 0x7FFF == 0
    assert s(ec.ONE, np.array([ec.NAN], np.uint16)) == (ec.NAN, ec.NAN)


# ---- (2) - (4) GELU ---------------------------------------------------------------------------------------------------------------------
def torch_gelu(x_bits):
    """torch's GELU on bf16; where |x| < 2^-125 or |x| >= 2^127 the same expression in fp32 torch ops (see the module docstring)."""
    x = t_bf16(x_bits)
    f = x.float()
    manual = ((f * 0.5) * (1.0 + torch.erf(f * 0.7071067811865476))).bfloat16()
    mag = np.asarray(x_bits, np.uint16) & 0x7FFF
    own = torch.from_numpy((mag < 0x0100) | (mag >= 0x7F00))
    return bits_of(torch.where(own, manual, torch.nn.functional.gelu(x)))


@pytest.mark.parametrize("n", ec.GELU_SIZES + (2 ** 18,))
def test_gelu_interval_holds_torch_and_decides_the_well_conditioned_regime(n):
    c = ec.gelu_case(n)
    iv = o.gelu(c["x"])
    got = torch_gelu(c["x"])
    assert int(iv.distance(got).max()) == 0, f"{n}: {iv.report(got)}"
    assert c["patterns"] == (n == 2 ** 18)
    if c["well"].any():
        share = iv.rows(c["well"]).decided_share()
        assert share >= ec.GELU_SHARE, f"{n}: {share:.4f} of the well-conditioned elements decided"


def test_gelu_all_patterns_and_degenerate_inputs():
    allp = o.all_bf16_patterns()
    iv = o.gelu(allp)
    got = torch_gelu(allp)
    assert int(iv.distance(got).max()) == 0, iv.report(got)
    und = ~iv.decided & ~iv.nan
    assert bool(((allp[und] >= 0x8000) | (allp[und] < 0x0100)).all())             # negative x, or x / 2 on a tie of the bf16 subnormal grid
    for x, want in ((0x0000, 0), (ec.POS_INF, ec.POS_INF), (ec.NEG_INF, ec.NAN), (ec.NAN, ec.NAN), (ec.MAX, ec.MAX), (0x4170, 0x4170)):
        assert (int(iv.lo[x]), int(iv.hi[x])) == (want, want), hex(x)
    for x in (ec.NEG_MAX, 0xC170):                                # (x / 2) * (1 - 1) = -0 is inside; the width is |x / 2| times erff's 8 u
        assert o.bf16_order(iv.lo[x]) <= 0 <= o.bf16_order(iv.hi[x]) and iv.v[x] == 0 and iv.rho[x] <= abs(o.bf16_to_f32(x)) * 2.0 ** -22, hex(x)
    pos = (allp < 0x7F80) & (allp >= 0x0100)
    assert iv.rows(pos).decided_share() >= 0.99                   # what the radius cannot decide is the negative tail


def test_past_the_clamp_cases_decide_their_well_conditioned_regime():
    c = ec.silu_case(*ec.SILU_PAST_CLAMP)
    assert c["patterns"] and o.silu_mul(c["gate"], c["up"]).rows(c["well"]).decided_share() >= ec.SILU_SHARE
    c = ec.gelu_case(ec.GELU_PAST_CLAMP)
    assert c["patterns"] and o.gelu(c["x"]).rows(c["well"]).decided_share() >= ec.GELU_SHARE


def test_past_the_clamp_sizes_are_past_the_clamp():
    """The arithmetic the GPU tests' docstring relies on."""
    B, S, Hq, Hk, D = ec.ROPE_PAST_CLAMP
    total = B * S * (Hq + Hk) * D // 8
    assert total > 256 * 32 * 256 and (total - 256 * 32 * 256) % 256 != 0
    for B, S, Hq, Hk, D in (ec.ROPE_FQ_PAST_CLAMP, ec.ROPE_VALUE_PAST_CLAMP):
        assert max(Hq, Hk) * D // 8 >= 256 and B * S > 256 * 64                # tpb = 1: one workgroup per token, more tokens than workgroups
    rows, cols = ec.SILU_PAST_CLAMP
    assert rows * cols // 8 > 256 * 32 * 256 and (rows * cols // 8) % 256 != 0
    assert ec.GELU_PAST_CLAMP // 8 > 256 * 32 * 256 and (ec.GELU_PAST_CLAMP // 8) % 256 != 0
