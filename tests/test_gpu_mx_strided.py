"""Microscaling along an axis that is not the last on the device: qt_quantize_mx_strided_* and qt_fake_quant_mx_strided_*
(csrc/qt_mx_quant.hip) through the C ABI, the fake-quant module, the quantized_ops operators, the PT2E fold and graph capture.

Every comparison is bit for bit with NaNs canonicalised, no tolerance.  The oracles:
  q, scale (quantize)    the CPU composite calculate_mx_qparam + quantize on x.cpu(): the reference's own op sequence
                         (decomposed.py:365-448), pinned by the PT2E goldens;
  y, scale (fake-quant)  oracle.qt_oracle.mx_fake_quant;
  codes, e8m0            oracle.qt_oracle.mx_pack on the transposed arrays.

recipe() draws randn * 2^randint(-20, 20) per column and plants an all-zero block, 255.0 (the bf16 logarithm rounds up to 8),
0.998, 2^-126, 3e38, +Inf, -Inf and NaN, each in a column and a block of its own where the shape has that many; -Inf and NaN sit in
the last row of their block, which the last row group of a workgroup holds."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_launch import Guarded, launch, nv, refused, stream  # noqa: F401
from mx_cases import (BF16, BITS, F32, IO_IDS, assert_same, bits_of, canon, cpu_pair, expected_pack, maps_for, oracle_fake_quant, qmax_of,
                      unpack_codes)
from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu


def view_of(shape, ax):
    ax %= len(shape)
    return int(np.prod(shape[:ax], dtype=np.int64)), shape[ax], int(np.prod(shape[ax + 1:], dtype=np.int64))


def recipe(shape, ax, bs, dtype, seed, extra=()):
    """-> (tensor of `dtype` on the CPU, planted (o, c) columns that hold a non-finite value)"""
    outer, n, inner = view_of(shape, ax)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(outer, n, inner, generator=g) * torch.exp2(torch.randint(-20, 20, (outer, 1, inner), generator=g).float())
    plants = [None, 255.0, 0.998, 2.0 ** -126, 3.0e38, float("inf"), -float("inf"), float("nan")] + list(extra)
    ncol, nblk = outer * inner, n // bs
    nonfinite = set()
    for i, v in enumerate(plants):
        col = (i * 3 + 1) % ncol                     # a column and a block of its own where there are that many
        oo, c, b = col // inner, col % inner, i % nblk
        if v is None:
            x[oo, b * bs:(b + 1) * bs, c] = 0.0
        else:
            row = b * bs + (bs - 1 if i in (6, 7) else 0)
            x[oo, row, c] = v
            if not np.isfinite(v):
                nonfinite.add((oo, c))
    return x.reshape(shape).to(dtype), nonfinite


def c_quantize(nv, x, ax, bs, fmt, lut, qmax, pow2, smap=None, pack=None, want_q=True, what=""):
    """qt_quantize_mx_strided_* into guarded buffers, twice -> dict of host arrays (q, s, codes, e8)."""
    outer, n, inner = view_of(tuple(x.shape), ax)
    npdt = np.uint16 if x.dtype == BF16 else np.uint32
    xd = x.cuda().contiguous()
    specs = {"s": ((outer, n // bs, inner), npdt)}
    if want_q:
        specs["q"] = ((outer, n, inner), npdt)
    if pack is not None:
        specs["codes"] = ((outer * inner, n * BITS[pack] // 8), np.uint8)
        specs["e8"] = ((outer * inner, n // 32), np.uint8)
    fn = getattr(nv.lib(), "qt_quantize_mx_strided_" + IO_IDS[x.dtype])

    def call(outs):
        return fn(xd.data_ptr(), outs["q"].ptr if want_q else None, outs["s"].ptr, outs["codes"].ptr if pack else None,
                  outs["e8"].ptr if pack else None, outer, n, inner, bs, ctypes.byref(fmt), lut.data_ptr(), qmax, int(pow2),
                  smap.data_ptr() if smap is not None else None, o.MX_ELEM[pack][0] if pack else -1, stream())
    out = launch(call, specs, what)
    return {k: (canon(v) if v.dtype != np.uint8 else v) for k, v in out.items()}


def c_fake_quant(nv, x, ax, bs, fmt, lut, qmax, pow2, smap=None, what=""):
    outer, n, inner = view_of(tuple(x.shape), ax)
    npdt = np.uint16 if x.dtype == BF16 else np.uint32
    xd = x.cuda().contiguous()
    fn = getattr(nv.lib(), "qt_fake_quant_mx_strided_" + IO_IDS[x.dtype])

    def call(outs):
        return fn(xd.data_ptr(), outs["y"].ptr, outs["s"].ptr, outer, n, inner, bs, ctypes.byref(fmt), lut.data_ptr(), qmax, int(pow2),
                  smap.data_ptr() if smap is not None else None, stream())
    out = launch(call, {"y": ((outer, n, inner), npdt), "s": ((outer, n // bs, inner), npdt)}, what)
    return {k: canon(v) for k, v in out.items()}


# ---- 1. layout sweep through the C ABI ----------------------------------------------------------------------------------------------
# the smallest shapes that reach each regime of the work decomposition: (shape, axis, block size)
LAYOUTS = [
    ((2, 3, 64, 40), 2, 32),      # 5 pieces per row, no power of two; dead lanes in the last workgroup
    ((1, 64, 8), 1, 8),           # one row group
    ((3, 1024, 16), 1, 512),      # 64 row groups
    ((2, 24, 16), 1, 12),         # ragged last row group
    ((5, 7, 8), 1, 1),            # a block is one row
    ((2, 24, 8, 16), 1, 12),      # inner = 128 over two trailing dimensions
]
FORMATS = [("fp8_e4m3", False), ("fp6_e3m2", False), ("fp4_e2m1", False), ("int8", False), ("posit8_1", True)]


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("name,row_form", FORMATS, ids=[f[0] for f in FORMATS])
def test_quantize_layout_sweep(nv, name, row_form, dtype, pow2):
    host, devm, fmt = maps_for(nv, name, row_form)
    qmax = qmax_of(name)
    for shape, ax, bs in LAYOUTS:
        x, _ = recipe(shape, ax, bs, dtype, seed=bs + len(shape))
        s_ref, q_ref = cpu_pair(x, ax, bs, host, qmax, pow2)
        got = c_quantize(nv, x, ax, bs, fmt, devm, qmax, pow2, what=f"{shape} bs={bs}")
        assert_same(got["s"], bits_of(s_ref), f"scale {shape} bs={bs}")
        assert_same(got["q"], bits_of(q_ref), f"q {shape} bs={bs}")


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("name,row_form", [("fp8_e4m3", False), ("posit8_1", True), ("int8", False)], ids=["fp8_e4m3", "posit8_1", "int8"])
def test_fake_quant_layout_sweep(nv, name, row_form, dtype, pow2):
    host, devm, fmt = maps_for(nv, name, row_form)
    qmax = qmax_of(name)
    for shape, ax, bs in LAYOUTS:
        x, _ = recipe(shape, ax, bs, dtype, seed=bs + len(shape))
        y_ref, s_ref = oracle_fake_quant(x, ax, bs, name, qmax, pow2)
        got = c_fake_quant(nv, x, ax, bs, fmt, devm, qmax, pow2, what=f"{shape} bs={bs}")
        assert_same(got["s"], s_ref, f"scale {shape} bs={bs}")
        assert_same(got["y"], y_ref, f"y {shape} bs={bs}")


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
def test_table_in_lds_from_four_million_elements(nv, dtype, pow2):
    """[8, 2048, 256] = 2^22 elements of a table format without the row form: the 1024-thread workgroups with the map in LDS, one per
    compute unit, each taking several trips (the only variant that passes the barrier at the end of a trip).  Both entry families,
    the reciprocal and the division path."""
    host, devm, fmt = maps_for(nv, "fp8_e4m3", False)
    shape, ax, bs = (8, 2048, 256), 1, 32
    x, _ = recipe(shape, ax, bs, dtype, seed=1)
    s_ref, q_ref = cpu_pair(x, ax, bs, host, 448.0, pow2)
    got = c_quantize(nv, x, ax, bs, fmt, devm, 448.0, pow2, what="LDS table, quantize")
    assert_same(got["s"], bits_of(s_ref), "scale")
    assert_same(got["q"], bits_of(q_ref), "q")
    # y = rd(q * s) with the composite's own q and s (what MXFakeQuantFunction computes from them)
    y_ref = q_ref * torch.repeat_interleave(s_ref, bs, dim=ax)
    got = c_fake_quant(nv, x, ax, bs, fmt, devm, 448.0, pow2, what="LDS table, fake-quant")
    assert_same(got["s"], bits_of(s_ref), "scale (fake-quant)")
    assert_same(got["y"], bits_of(y_ref), "y")


def test_every_positive_finite_bf16_amax(nv):
    """floor(log2(amax)) is taken of the bf16-ROUNDED logarithm: one column per pattern 1 .. 0x7F7F (and one column of zeros, which
    makes the row length a multiple of 8)."""
    host, devm, fmt = maps_for(nv, "fp8_e4m3", False)
    pats = np.arange(1, 0x7F80, dtype=np.uint16)
    assert len(pats) == 32639
    x = torch.zeros(32, 32640, dtype=BF16)
    x[0, :len(pats)] = torch.from_numpy(pats.view(np.int16)).view(BF16)
    s_ref, q_ref = cpu_pair(x, 0, 32, host, 448.0, True)
    got = c_quantize(nv, x, 0, 32, fmt, devm, 448.0, True, what="every amax")
    assert_same(got["s"], bits_of(s_ref), "scale")
    assert_same(got["q"], bits_of(q_ref), "q")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
def test_scale_map(nv, dtype):
    host, devm, fmt = maps_for(nv, "fp4_e2m1", False)
    shost, sdev, _ = maps_for(nv, "fp8_e4m3", False)
    x = (torch.randn(32, 128, generator=torch.Generator().manual_seed(2)) * 3).to(dtype)
    s_ref, q_ref = cpu_pair(x, 0, 16, host, 6.0, False, shost)
    got = c_quantize(nv, x, 0, 16, fmt, devm, 6.0, False, smap=sdev, what="scale map")
    assert_same(got["s"], bits_of(s_ref), "scale")
    assert_same(got["q"], bits_of(q_ref), "q")
    y_ref, s_ref = oracle_fake_quant(x, 0, 16, "fp4_e2m1", 6.0, False, "fp8_e4m3")
    got = c_fake_quant(nv, x, 0, 16, fmt, devm, 6.0, False, smap=sdev, what="scale map, fake-quant")
    assert_same(got["s"], s_ref, "scale (fake-quant)")
    assert_same(got["y"], y_ref, "y")


# ---- 2. the packed operand ---------------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(3, 64, 80), (1, 32, 24), (2, 160, 16), (2, 192, 16)]     # [B, K, N]; K = 160, 192: a multi-block tile ends ragged


@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("name", sorted(BITS))
def test_pack_equals_the_host_packer(nv, name, dtype):
    host, devm, fmt = maps_for(nv, name, False)
    qmax = qmax_of(name)
    qe = int(np.floor(np.log2(qmax)))
    seen_flush = 0
    for shape in PACK_SHAPES:
        B, K, N = shape
        if (K * BITS[name] // 8) % 16:
            assert BITS[name] == 6 and K in (32, 160)             # 24 and 120 bytes: the entry point declines, tested below
            continue
        # a column whose amax gives the scale 2^-130 (below E8M0's 2^-127), and the issue's 2^-140 (fp32 only: bf16 has no such value)
        x, nonfinite = recipe(shape, 1, 32, dtype, seed=K + N, extra=(2.0 ** (qe - 130), 2.0 ** -140))
        xv = x.view(B, K, N)
        for i in (8, 9):                                          # the two extra plants: the rest of their block is zero
            col, b = (i * 3 + 1) % (B * N), i % (K // 32)
            keep = xv[col // N, b * 32, col % N].clone()
            xv[col // N, b * 32:(b + 1) * 32, col % N] = 0.0
            xv[col // N, b * 32, col % N] = keep
        s_ref, q_ref = cpu_pair(x, 1, 32, host, qmax, True)
        want_codes, want_e8, rows, nflush = expected_pack(s_ref, q_ref, name, 32)
        seen_flush += nflush
        left_out = B * N - len(rows)
        print(f"[pack {name} {IO_IDS[dtype]} {shape}] {left_out} of {B * N} columns ({left_out / (B * N):.2%}) left out of the comparison, "
              f"{len(nonfinite)} hold a planted Inf / NaN; {nflush} blocks flushed")
        assert left_out <= len(nonfinite), f"{shape}: {left_out} of {B * N} columns left out, {len(nonfinite)} planted non-finite"
        for want_q in (True, False):
            got = c_quantize(nv, x, 1, 32, fmt, devm, qmax, True, pack=name, want_q=want_q, what=f"pack {shape} q={want_q}")
            assert_same(got["s"], bits_of(s_ref), f"scale {shape}")
            if want_q:
                assert_same(got["q"], bits_of(q_ref), f"q {shape}")
            assert_same(got["codes"][rows], want_codes, f"codes {shape} q={want_q}")
            assert_same(got["e8"][rows], want_e8, f"e8m0 {shape} q={want_q}")
        got = c_quantize(nv, x, 1, 32, fmt, devm, qmax, True, want_q=False, what=f"scales only {shape}")
        assert_same(got["s"], bits_of(s_ref), f"scales only {shape}")
    assert seen_flush >= 1, "no block was flushed: the plant did not reach the rule"


def test_pack_with_blocks_of_64_and_96(nv):
    """Blocks wider than 32 repeat their E8M0 byte; 96 rows make 16 row groups of 6 rows, whose codes go to LDS byte by byte."""
    host, devm, fmt = maps_for(nv, "fp8_e4m3", False)
    for bs, shape in ((64, (2, 128, 24)), (96, (1, 192, 16))):
        x, _ = recipe(shape, 1, bs, BF16, seed=bs)
        s_ref, q_ref = cpu_pair(x, 1, bs, host, 448.0, True)
        want_codes, want_e8, rows, _ = expected_pack(s_ref, q_ref, "fp8_e4m3", bs)
        got = c_quantize(nv, x, 1, bs, fmt, devm, 448.0, True, pack="fp8_e4m3", what=f"pack bs={bs}")
        assert_same(got["q"], bits_of(q_ref), f"q bs={bs}")
        assert_same(got["codes"][rows], want_codes, f"codes bs={bs}")
        assert_same(got["e8"][rows], want_e8, f"e8m0 bs={bs}")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("name", sorted(BITS))
def test_a_non_finite_element_stays_in_its_own_bits(nv, name, dtype):
    """A code row that holds an Inf or a NaN: every FINITE element of it still carries exactly its own code -- in the strided kernel,
    where the neighbouring code belongs to another operand row, and in the last-axis kernel, which packs through the same helper
    (qt_mx::vec_codes masks each code to its width; the 6-bit formats and every fp32 tensor take the path that needs it)."""
    from quantized_training import mx_operand
    from quantized_training.fake_quantize import get_quantization_map
    host, qmap = get_quantization_map(name, "cpu"), get_quantization_map(name, "cuda")
    qmax, bits = qmax_of(name), BITS[name]
    b = torch.randn(2, 64, 32, generator=torch.Generator().manual_seed(4))
    b[0, 5, 3], b[1, 40, 7], b[0, 63, 31] = float("inf"), float("nan"), -float("inf")
    b = b.to(dtype)
    a = b.transpose(1, 2).contiguous()                            # the same blocks along the last axis
    for what, x, ax, layout in (("strided", b, -2, mx_operand.SECOND), ("last axis", a, -1, mx_operand.ROWS)):
        s_ref, q_ref = cpu_pair(x, ax, 32, host, qmax, True)
        s, q = torch.ops.quantized_ops.quantize_mx(x.cuda(), qmap, [ax], 32, qmax, True, None, None)
        assert_same(bits_of(q), bits_of(q_ref), f"{what}: q")
        rows = (q_ref.transpose(1, 2) if ax == -2 else q_ref).reshape(64, 64).float().numpy()
        finite = np.isfinite(rows)
        assert int((~finite.all(axis=1)).sum()) == 3, f"{what}: three code rows hold a non-finite value"
        got = unpack_codes(mx_operand.operand_record(q, layout)[2].cpu().numpy(), bits)
        assert got.shape == (64, 64)
        assert_same(got[finite], o.mx_encode(rows[finite], name), f"{what}: codes of the finite elements")
        assert int(got.max()) < (1 << bits)


# ---- 3. refusals on the device: nothing is written ------------------------------------------------------------------------------------
HUGE = 2 ** 35                                       # inner / 8 and inner / 4 above 2^32 - 1
# every decline of the entry points (include/qt_hip.h), as overrides of a call that would be taken
DECLINES = {
    "NULL x": dict(x="null"), "NULL scales": dict(s="null"), "NULL fmt": dict(fmt=False), "table format without a table": dict(lut=False),
    "block size 0": dict(bs=0), "block size 513": dict(bs=513, n=1026), "quant_max 0": dict(qmax=0.0), "quant_max negative": dict(qmax=-1.0),
    "inner 1": dict(inner=1), "inner above 2^32 - 1 vectors": dict(inner=HUGE),
    "n % block_size": dict(n=72), "inner off the vector": dict(inner=34),
    "x off 16 bytes": dict(x="off"), "q off 16 bytes": dict(q="off"), "scales off 16 bytes": dict(s="off"),
}
PACK_DECLINES = {
    "codes without e8m0": dict(e8="null"), "e8m0 without codes": dict(codes="null"), "pack without force_pow2": dict(pow2=0),
    "pack_format 5": dict(pf=5), "pack_format -1": dict(pf=-1), "pack with block size 16": dict(bs=16),
    "pack with block size 48": dict(bs=48, n=96), "codes off 16 bytes": dict(codes="off"), "e8m0 off 16 bytes": dict(e8="off"),
    "code row of 24 bytes": dict(n=32, pf=2), "code row of 72 bytes": dict(n=96, pf=3),
}


@pytest.mark.parametrize("io", ["bf16", "f32"])
def test_refusals_write_nothing(nv, io):
    host, devm, fmt = maps_for(nv, "fp8_e4m3", False)
    L = nv.lib()
    npdt = np.uint16 if io == "bf16" else np.uint32
    x = torch.randn(2 * 64 * 32 + 64, device="cuda").to(BF16 if io == "bf16" else F32)
    full = {"q": ((2, 64, 32), npdt), "s": ((2, 2, 32), npdt), "codes": ((64, 64), np.uint8), "e8": ((64, 2), np.uint8)}

    def pointer(base, mode):
        return {"ok": base, "null": None, "off": base + 8}[mode]

    def call_of(family, **kw):
        a = dict(x="ok", q="ok", s="ok", codes="ok", e8="ok", outer=2, n=64, inner=32, bs=32, fmt=True, lut=True, qmax=448.0, pow2=1, pf=0)
        a.update(kw)
        F, lut = (ctypes.byref(fmt) if a["fmt"] else None), (devm.data_ptr() if a["lut"] else None)

        def call(outs):
            xp, qp, sp = pointer(x.data_ptr(), a["x"]), pointer(outs["q"].ptr, a["q"]), pointer(outs["s"].ptr, a["s"])
            if family == "quantize":
                return getattr(L, "qt_quantize_mx_strided_" + io)(xp, qp, sp, pointer(outs["codes"].ptr, a["codes"]), pointer(outs["e8"].ptr, a["e8"]),
                                                                  a["outer"], a["n"], a["inner"], a["bs"], F, lut, a["qmax"], a["pow2"], None,
                                                                  a["pf"], stream())
            return getattr(L, "qt_fake_quant_mx_strided_" + io)(xp, qp, sp, a["outer"], a["n"], a["inner"], a["bs"], F, lut, a["qmax"], a["pow2"],
                                                                None, stream())
        return call

    for what, kw in {**DECLINES, **PACK_DECLINES}.items():
        refused(call_of("quantize", **kw), full, f"quantize_{io}: {what}")
    for what, kw in DECLINES.items():                             # without a pack the same declines hold
        refused(call_of("quantize", codes="null", e8="null", **kw), {"q": full["q"], "s": full["s"], "codes": full["codes"], "e8": full["e8"]},
                f"quantize_{io}, no pack: {what}")
    for what, kw in {**DECLINES, "NULL y": dict(q="null")}.items():
        refused(call_of("fake_quant", **kw), {"q": full["q"], "s": full["s"]}, f"fake_quant_{io}: {what}")


# ---- 4. the module ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow2", [False, True], ids=["amax", "pow2"])
def test_module_equals_its_cpu_twin(nv, pow2):
    from dataclasses import asdict
    import quantized_training as qt
    kw = asdict(qt.QuantizationSpec.from_str("fp8_e4m3,qs=microscaling,bs=32,ax=-2"))
    x, _ = recipe((2, 4, 64, 32), 2, 32, BF16, seed=3)
    m_cpu = qt.FusedAmaxObsFakeQuantize(**kw, force_scale_power_of_two=pow2)
    m_dev = qt.FusedAmaxObsFakeQuantize(**kw, force_scale_power_of_two=pow2, device="cuda")
    xd = x.cuda().requires_grad_(True)
    y_dev = m_dev(xd)
    y_cpu = m_cpu(x)
    assert_same(bits_of(y_dev), bits_of(y_cpu), "y")
    assert m_dev.scale.shape == m_cpu.scale.shape == (2, 4, 2, 32)
    assert_same(bits_of(m_dev.scale), bits_of(m_cpu.scale), "scale buffer")
    g = torch.randn_like(y_dev)
    y_dev.backward(g)
    assert torch.equal(xd.grad, g)                               # straight through


# ---- 5. the operators ---------------------------------------------------------------------------------------------------------------------
def test_quantize_mx_operator_and_the_matmul_operand(nv):
    from quantized_training import mx_gemm, mx_operand
    from quantized_training.fake_quantize import get_quantization_map
    host, qmap = get_quantization_map("fp8_e4m3", "cpu"), get_quantization_map("fp8_e4m3", "cuda")
    g = torch.Generator().manual_seed(5)
    a = torch.randn(3, 96, 64, generator=g).bfloat16().cuda()
    b = torch.randn(3, 64, 80, generator=g).bfloat16()
    s_ref, q_ref = cpu_pair(b, -2, 32, host, 448.0, True)
    sb, qb = torch.ops.quantized_ops.quantize_mx(b.cuda(), qmap, [-2], 32, 448.0, True, None, None)
    assert_same(bits_of(sb), bits_of(s_ref), "scale")
    assert_same(bits_of(qb), bits_of(q_ref), "q")
    fid, bs, codes, e8 = mx_operand.operand_record(qb, mx_operand.SECOND)
    assert (fid, bs, tuple(codes.shape), tuple(e8.shape)) == (0, 32, (3 * 80, 64), (3 * 80, 2))
    want_codes, want_e8, rows, _ = expected_pack(s_ref, q_ref, "fp8_e4m3", 32)
    assert len(rows) == 3 * 80
    assert_same(codes.cpu().numpy(), want_codes, "codes")
    assert_same(e8.cpu().numpy(), want_e8, "e8m0")
    assert mx_operand.is_pow2(sb) and mx_operand.format_of(qb) == "fp8_e4m3"

    sa, qa = torch.ops.quantized_ops.quantize_mx(a, qmap, [-1], 32, 448.0, True, None, None)
    mx_gemm.STATS.reset()
    y1 = torch.ops.quantized_ops.matmul_mx(qa, qb, input_scale=sa, weight_scale=sb, block_size=32)
    mx_operand.drop_operand(qb)                                 # the qt_mx_pack route
    y2 = torch.ops.quantized_ops.matmul_mx(qa, qb, input_scale=sa, weight_scale=sb, block_size=32)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 0)
    assert_same(bits_of(y1), bits_of(y2), "matmul_mx with the operand of quantize_mx against the strided pack")

    s_only = torch.ops.quantized_ops.calculate_mx_qparam(b.cuda(), [-2], 32, 448.0, True)
    assert_same(bits_of(s_only), bits_of(s_ref), "calculate_mx_qparam")
    assert mx_operand.is_pow2(s_only)
    s_amax = torch.ops.quantized_ops.calculate_mx_qparam(b.cuda(), [-2], 32, 448.0, False)
    assert_same(bits_of(s_amax), bits_of(torch.ops.quantized_ops.calculate_mx_qparam(b, [-2], 32, 448.0, False)), "calculate_mx_qparam, amax")


def test_transposed_view_runs_the_last_axis_pass(nv):
    from quantized_training import mx_operand
    from quantized_training.fake_quantize import get_quantization_map
    host, qmap = get_quantization_map("fp8_e4m3", "cpu"), get_quantization_map("fp8_e4m3", "cuda")
    k = torch.randn(2, 4, 96, 64, generator=torch.Generator().manual_seed(9)).bfloat16()
    kt = k.transpose(-1, -2)
    s_ref, q_ref = cpu_pair(kt, -2, 32, host, 448.0, True)
    s, q = torch.ops.quantized_ops.quantize_mx(k.cuda().transpose(-1, -2), qmap, [-2], 32, 448.0, True, None, None)
    assert s.shape == s_ref.shape and q.shape == q_ref.shape
    assert_same(bits_of(s), bits_of(s_ref), "scale")
    assert_same(bits_of(q), bits_of(q_ref), "q")
    s1, q1 = torch.ops.quantized_ops.quantize_mx(k.cuda(), qmap, [-1], 32, 448.0, True, None, None)
    for got, want in zip(mx_operand.operand_record(q, mx_operand.SECOND), mx_operand.operand_record(q1, mx_operand.ROWS)):
        assert torch.equal(got, want) if isinstance(got, torch.Tensor) else got == want
    assert mx_operand.operand_record(q, mx_operand.SECOND)[2].shape == (2 * 4 * 96, 64)


# ---- 6. PT2E ------------------------------------------------------------------------------------------------------------------------------
def _device_converted(name, native):
    import os
    import test_pt2e_cpu as t
    from quantized_training import quantize_pt2e as qp
    arr = np.load(os.path.join(t.G, "pt2e_mx.npz"))
    info, m, xs = t.mx_setup(name, arr, device="cuda")
    gm = qp.prepare_pt2e(m, qp.get_default_quantizer(**info["kw"]), (xs[0],))
    with torch.no_grad():
        gm(xs[0])
        gm(xs[1])
        gc = qp.convert_pt2e(gm, native=native)
        y = gc(xs[1])
    return gc, y, arr[f"{name}__y_converted"], t


def _mx_configs():
    import json
    import os
    return sorted(json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pt2e_mx.json"))))


@pytest.mark.parametrize("name", _mx_configs())
def test_pt2e_fold_does_not_change_the_device_result(nv, name):
    gc_f, y_f, golden, t = _device_converted(name, native=True)
    gc_u, y_u, _, _ = _device_converted(name, native=False)
    ops = torch.ops.quantized_ops
    assert not [n for n in gc_f.graph.nodes if n.op == "call_function" and n.target == ops.calculate_mx_qparam.default and n.args[0].op != "get_attr"]
    assert [n for n in gc_u.graph.nodes if n.op == "call_function" and n.target == ops.calculate_mx_qparam.default and n.args[0].op != "get_attr"]
    for tag, y in (("folded", y_f), ("unfolded", y_u)):           # reported only: the device GEMM accumulates in another order than the CPU
        b = t._bits(y.cpu())
        differ = b != golden
        yf = y.float().cpu().numpy().reshape(-1)
        gf = (o.bf16_to_f32(golden.reshape(-1)) if golden.dtype == np.uint16 else golden.reshape(-1).view(np.float32))
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(yf - gf))) if differ.any() else 0.0
        print(f"[pt2e {name}] {tag}: {differ.mean():.4%} of the elements differ from the golden y_converted, largest difference {worst:.3g}")
    assert_same(bits_of(y_f), bits_of(y_u), "folded against unfolded")


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------
def test_graph_capture_replays_the_eager_result(nv):
    host, devm, fmt = maps_for(nv, "fp8_e4m3", False)
    L = nv.lib()
    B, K, N = 2, 64, 48
    x = torch.randn(B, K, N, device="cuda").bfloat16()
    F = ctypes.byref(fmt)

    def buffers():
        return (torch.zeros(B, K, N, dtype=BF16, device="cuda"), torch.zeros(B, K // 32, N, dtype=BF16, device="cuda"),
                torch.zeros(B * N, K, dtype=torch.uint8, device="cuda"), torch.zeros(B * N, K // 32, dtype=torch.uint8, device="cuda"),
                torch.zeros(B, K, N, dtype=BF16, device="cuda"), torch.zeros(B, K // 32, N, dtype=BF16, device="cuda"))

    def run(q, s, codes, e8, y, sy):
        st = stream()
        assert L.qt_quantize_mx_strided_bf16(x.data_ptr(), q.data_ptr(), s.data_ptr(), codes.data_ptr(), e8.data_ptr(), B, K, N, 32, F,
                                             devm.data_ptr(), 448.0, 1, None, 0, st) == 0
        assert L.qt_fake_quant_mx_strided_bf16(x.data_ptr(), y.data_ptr(), sy.data_ptr(), B, K, N, 32, F, devm.data_ptr(), 448.0, 0, None, st) == 0

    eager = buffers()
    run(*eager)
    torch.cuda.synchronize()
    captured = buffers()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):                    # one stream, no parallel branches
            run(*captured)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t_ in captured:
            t_.zero_()
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
