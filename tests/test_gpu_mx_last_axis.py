"""Microscaling along the LAST axis on the device: qt_quantize_mx_bf16 / _f32 (csrc/qt_mx_quant.hip, quantize_mx_kernel) and
qt_fake_quant_mx_bf16 / _f32 (csrc/qt_elementwise.hip, fq_mx_kernel), every variant through the C ABI, and once through the operator.

Every comparison is bit for bit with NaNs canonicalised, no tolerance, no element left out but the code rows named in (d).  Oracles:
  q, scales (quantize)      the CPU composite calculate_mx_qparam + quantize on x.cpu(): the reference's own op sequence;
  y, scales (fake-quant)    oracle.qt_oracle.mx_fake_quant;
  codes, e8m0               oracle.qt_oracle.mx_pack, a scale below 2^-127 restated as codes 0 and byte 0 (mx_cases.expected_pack_rows).

recipe() draws randn * 2^randint(-20, 20) per row and plants an all-zero block, 255.0 (the bf16 logarithm rounds up to 8), 0.998,
2^-126, 3e38, +Inf, -Inf and NaN, each in a row and a block of its own where the shape has that many; -Inf and NaN sit in the last
element of their block, which the block's last lane holds.  `alone` plants are their block's only non-zero element: 2^-110 (a scale
below UniformDiv's band of 2^-100 .. 2^100: the exact division), 2^-140 (fp32: a subnormal scale) and 2^(qe - 130) (the flush rule).

kPer = 8 (bf16) / 4 (fp32) elements of a 16-byte vector; one lane takes one vector, group = block / kPer adjacent lanes reduce the
block's amax by __shfl_xor; nvec = rows cols / kPer; CU = compute units of the device (read at run time).  Constants restated from csrc:
WG_PER_CU = 32 (launch_pb's `cap`, launch_mx's grid_for(nvec, 256, 32)), LDS_MIN = 2^22 elements (launch: `lds`).

Which element pass of quantize_mx_kernel<IO, LDS_TABLE, PACK_BITS, ROWS> a launch takes (launch, launch_pb):
  ROWS       a table format whose qt_format carries the row bit (p1 & 1)                         256 threads, <= 32 CU workgroups
  LDS_TABLE  a table format without the row bit from LDS_MIN elements, table on 16 bytes         1024 threads, CU workgroups
  global     a table format without the row bit below LDS_MIN (or the table off 16 bytes)        256 threads, <= 32 CU workgroups
  closed     fmt->kind != QT_FMT_LUT (nv.format_for("int8") = QT_FMT_INT, "e4m3" = QT_FMT_FP_SAT)   the global kernel with lut == NULL
fq_mx_kernel<IO, KIND>: KIND = fmt->kind, QT_FMT_LUT (the row bit is ignored: the table is gathered), FP_SAT, INT, IDENTITY.

  case                              entry point          variant                                   why this size reaches it
  --------------------------------  -------------------  ----------------------------------------  ----------------------------------------------
  a test_quantize_block_sweep       qt_quantize_mx_*     IO x {global, ROWS, closed INT, closed    3 rows x 5 blocks at group 1 (no shuffle) .. 64
                                                         FP_SAT} x PACK 0, pow2 and amax           (the whole wave); 3 x 43 blocks at group 4 =
  a test_fake_quant_block_sweep     qt_fake_quant_mx_*   IO x {LUT, LUT + row bit, INT, FP_SAT,    516 vectors: two full workgroups and one with 4
                                                         IDENTITY}; fast and exact division        live lanes (ragged).  All below LDS_MIN
  b test_table_in_lds               qt_quantize_mx_*     IO x LDS_TABLE x PACK {0, 8, 6, 4}        >= LDS_MIN elements and > CU 1024 vectors: at
                                                                                                   least two trips, the last with a ragged wave
  c test_second_trip_quantize       qt_quantize_mx_bf16  ROWS x PACK 8; global x PACK 0 (table     nvec = WG_PER_CU CU 256 + 3 256 + group: every
                                                         off 16 bytes); closed INT x PACK 0        workgroup makes a second trip, live only in
  c test_second_trip_fake_quant     qt_fake_quant_mx_*   f32 INT; bf16 LUT, FP_SAT, IDENTITY       three workgroups and `group` lanes of a fourth
  d test_pack_equals_the_host_      qt_quantize_mx_*     IO x {global, ROWS where the device map   12 rows of K = 64, 160, 192 at block 32; blocks
    packer                                               carries one, closed FP_SAT for e4m3} x    64, 128, 512 (256 fp32) repeat the E8M0 byte;
                                                         PACK {8, 6, 4}, all five QT_MX_*,         q_dev given and NULL; below LDS_MIN
                                                         q_dev given and NULL
  e test_every_f32_binade           qt_quantize_mx_f32   global, kMxLog2ThrF32 and the subnormal   quant_max = 1: scale = 2^floor(log2 amax), one
                                                         branch of floor_log2_dtype                block of 4 per amax pattern
  f test_scale_map                  both families        global / LUT with scale_lut               fp4_e2m1 elements, fp8_e4m3 scales, block 16
  g test_operator_at_the_lds_size   quantize_mx (op)     whichever the product picks x PACK 8      one bf16 tensor of >= LDS_MIN elements
  h test_refusals_write_nothing     all four             every decline of launch and launch_mx     nothing is launched

closed x PACK {6, 4} is compiled but no format reaches it: qt_format_for gives the 6- and 4-bit formats as tables.  The large cases (b,
c, g) tile a recipe of a prime number of rows and evaluate the expectation on one period: blocks never cross rows, so that is exact."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_launch import Guarded, launch, nv, refused, stream  # noqa: F401
from mx_cases import (BF16, BITS, F32, IO_IDS, assert_same, bits_of, canon, cpu_pair, expected_pack_rows, f32_binade_patterns, maps_for,
                      oracle_fake_quant, qmax_of, unpack_codes)
from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

KPER = {BF16: 8, F32: 4}
WG_PER_CU = 32                     # csrc/qt_mx_quant.hip launch_pb: cap = qt_cu_count() * 32; csrc/qt_elementwise.hip launch_mx: grid_for(nvec, 256, 32)
LDS_MIN = 1 << 22                  # csrc/qt_mx_quant.hip launch: lds = ... rows * cols >= ((size_t)1 << 22)
LDS_THREADS = 1024                 # one workgroup of 1024 per compute unit
PERIOD = 4099                      # rows of the recipe the large cases tile: a prime, so a row meets every lane position
QMAX = {"e4m3": 448.0, "int8": 127.0, None: 448.0}
PLANTS = [None, 255.0, 0.998, 2.0 ** -126, 3.0e38, float("inf"), -float("inf"), float("nan")]


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def qmax_for(name):
    return QMAX[name] if name in QMAX else qmax_of(name)


def recipe(rows, nblk, bs, dtype, seed, alone=()):
    """-> (tensor [rows, nblk bs] of `dtype` on the CPU, the rows that hold a planted Inf / NaN)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, nblk * bs, generator=g) * torch.exp2(torch.randint(-20, 20, (rows, 1), generator=g).float())
    nonfinite = set()
    for i, v in enumerate(PLANTS + list(alone)):
        r = i % rows                                    # a row and a block of its own where there are that many
        b = (i // rows + r) % nblk
        blk = x[r, b * bs:(b + 1) * bs]
        if v is None or i >= len(PLANTS):
            blk.zero_()
        if v is not None:
            blk[bs - 1 if i in (6, 7) else 0] = v
            if not np.isfinite(v):
                nonfinite.add(r)
    return x.to(dtype), nonfinite


def tile_rows(a, total):
    """the first `total` rows of a [period, ...] array or tensor repeated along the rows"""
    reps = -(-total // a.shape[0])
    if isinstance(a, torch.Tensor):
        return a.repeat(reps, *([1] * (a.dim() - 1)))[:total].contiguous()
    return np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:total]


def form_of(nv, name, kind):
    """-> (host map or None, qt_format, device table or None).  kind: table (no row bit) | rows | closed | identity | misaligned
    (the table 8 bytes off a 16-byte boundary: neither the row form nor the table in LDS is taken)"""
    from quantized_training.fake_quantize import get_quantization_map
    if kind == "identity":
        return None, nv.format_for(None), None
    if kind == "closed":
        fmt = nv.format_for(name)
        assert fmt.kind != nv.QT_FMT_LUT, f"{name} has no closed form"
        return get_quantization_map(name, "cpu"), fmt, None
    host, devm, fmt = maps_for(nv, name, kind == "rows")
    if kind == "misaligned":
        buf = torch.empty(devm.numel() + 8, dtype=devm.dtype, device="cuda")
        devm = buf[4:4 + devm.numel()].copy_(devm)
        assert devm.data_ptr() % 16 == 8
    return host, fmt, devm


def has_row_form(name):
    from quantized_training.fake_quantize import get_quantization_map
    return bool(getattr(get_quantization_map(name, "cuda"), "_qt_rows", 0) & 1)


def c_quantize(nv, x, bs, fmt, lut, qmax, pow2, smap=None, pack=None, want_q=True, what=""):
    """qt_quantize_mx_* into guarded buffers, twice -> dict of host arrays (q, s, codes, e8)."""
    rows, cols = x.shape
    npdt = np.uint16 if x.dtype == BF16 else np.uint32
    xd = x.cuda().contiguous()
    specs = {"s": ((rows, cols // bs), npdt)}
    if want_q:
        specs["q"] = ((rows, cols), npdt)
    if pack is not None:
        specs["codes"] = ((rows, cols * BITS[pack] // 8), np.uint8)
        specs["e8"] = ((rows, cols // 32), np.uint8)
    fn = getattr(nv.lib(), "qt_quantize_mx_" + IO_IDS[x.dtype])

    def call(outs):
        return fn(xd.data_ptr(), outs["q"].ptr if want_q else None, outs["s"].ptr, outs["codes"].ptr if pack else None,
                  outs["e8"].ptr if pack else None, rows, cols, bs, ctypes.byref(fmt), lut.data_ptr() if lut is not None else None, qmax,
                  int(pow2), smap.data_ptr() if smap is not None else None, o.MX_ELEM[pack][0] if pack else -1, stream())
    out = launch(call, specs, what)
    return {k: (canon(v) if v.dtype != np.uint8 else v) for k, v in out.items()}


def c_fake_quant(nv, x, bs, fmt, lut, qmax, smap=None, what=""):
    rows, cols = x.shape
    npdt = np.uint16 if x.dtype == BF16 else np.uint32
    xd = x.cuda().contiguous()
    fn = getattr(nv.lib(), "qt_fake_quant_mx_" + IO_IDS[x.dtype])

    def call(outs):
        return fn(xd.data_ptr(), outs["y"].ptr, outs["s"].ptr, rows, cols, bs, ctypes.byref(fmt), lut.data_ptr() if lut is not None else None,
                  qmax, smap.data_ptr() if smap is not None else None, stream())
    out = launch(call, {"y": ((rows, cols), npdt), "s": ((rows, cols // bs), npdt)}, what)
    return {k: canon(v) for k, v in out.items()}


def pack_expectation(s_ref, q_ref, name, bs):
    """-> (codes, e8m0, keep, values, flushed blocks) for [rows, K]: every row, the rows left out of the comparison as zeros; keep[r]:
    row r is compared; values: q with the flushed blocks as zeros (what the finite elements of the other rows must still encode)."""
    qt = q_ref.float().numpy().astype(np.float64)
    st = s_ref.float().numpy().astype(np.float64)
    codes, e8, rows, nflush = expected_pack_rows(qt, st, name, bs)
    full_codes = np.zeros((qt.shape[0], codes.shape[1]), np.uint8)
    full_e8 = np.zeros((qt.shape[0], e8.shape[1]), np.uint8)
    keep = np.zeros(qt.shape[0], bool)
    full_codes[rows], full_e8[rows], keep[rows] = codes, e8, True
    values = qt.copy()
    with np.errstate(invalid="ignore"):
        values[np.repeat(st < 2.0 ** -127, bs, axis=1)] = 0.0
    return full_codes, full_e8, keep, values, nflush


# ---- a. block sweep: both ends of the shuffle reduction, a ragged last workgroup ------------------------------------------------------------
GROUPS = (1, 2, 4, 8, 16, 32, 64)
SWEEP = [(3, 5, g) for g in GROUPS] + [(3, 43, 4)]          # (rows, blocks per row, lanes per block); the last: 516 vectors
Q_FORMS = [("fp8_e4m3", "table"), ("posit8_1", "rows"), ("int8", "closed"), ("e4m3", "closed")]
FQ_FORMS = Q_FORMS + [(None, "identity")]


def form_id(f):
    return f"{f[0]}-{f[1]}"


def sweep_alone(dtype):
    return (2.0 ** -110,) + ((2.0 ** -140,) if dtype == F32 else ())


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("form", Q_FORMS, ids=form_id)
def test_quantize_block_sweep(nv, form, dtype, pow2):
    host, fmt, lut = form_of(nv, *form)
    qmax = qmax_for(form[0])
    for rows, nblk, group in SWEEP:
        bs = group * KPER[dtype]
        assert rows * nblk * bs < LDS_MIN
        x, _ = recipe(rows, nblk, bs, dtype, seed=group + nblk, alone=sweep_alone(dtype))
        s_ref, q_ref = cpu_pair(x, -1, bs, host, qmax, pow2)
        got = c_quantize(nv, x, bs, fmt, lut, qmax, pow2, what=f"[{rows}, {nblk} x {bs}]")
        assert_same(got["s"], bits_of(s_ref), f"scale [{rows}, {nblk} x {bs}]")
        assert_same(got["q"], bits_of(q_ref), f"q [{rows}, {nblk} x {bs}]")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("form", FQ_FORMS, ids=form_id)
def test_fake_quant_block_sweep(nv, form, dtype):
    _, fmt, lut = form_of(nv, *form)
    qmax = qmax_for(form[0])
    exact = 0
    for rows, nblk, group in SWEEP:
        bs = group * KPER[dtype]
        x, _ = recipe(rows, nblk, bs, dtype, seed=group + nblk, alone=sweep_alone(dtype))
        y_ref, s_ref = oracle_fake_quant(x, -1, bs, form[0], qmax, False)
        got = c_fake_quant(nv, x, bs, fmt, lut, qmax, what=f"[{rows}, {nblk} x {bs}]")
        assert_same(got["s"], s_ref, f"scale [{rows}, {nblk} x {bs}]")
        assert_same(got["y"], y_ref, f"y [{rows}, {nblk} x {bs}]")
        band = (s_ref.astype(np.uint32) << 16 if s_ref.dtype == np.uint16 else s_ref) & 0x7FFFFFFF
        exact += int((band < ((127 - 100) << 23)).sum())                 # UniformDiv::safe: 2^-100 <= s <= 2^100
        if dtype == F32 and qmax < 1024.0:                               # (2^-140 / 4096 rounds to 0, which the where() guard makes 1)
            assert (band < (1 << 23)).any(), "no block has a subnormal scale"
    assert exact >= len(SWEEP), "no block has a scale below UniformDiv's band"


# ---- b. the table in LDS --------------------------------------------------------------------------------------------------------------------
def lds_rows(cols, kper):
    """rows of a [rows, cols] tensor of at least LDS_MIN elements whose vectors make at least two trips of CU workgroups of 1024, the last
    one ragged down to the wave"""
    per_trip = cus() * LDS_THREADS
    rows = -(-max(LDS_MIN, per_trip * kper + 1) // cols)
    while (rows * cols // kper) % 64 == 0 or (rows * cols // kper) % per_trip == 0:
        rows += 1
    return rows


@pytest.mark.parametrize("pow2", [True, False], ids=["pow2", "amax"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
def test_table_in_lds(nv, dtype, pow2):
    cols, bs = 160, 32
    rows = lds_rows(cols, KPER[dtype])
    nvec = rows * cols // KPER[dtype]
    assert rows * cols >= LDS_MIN and nvec > cus() * LDS_THREADS and nvec % (cus() * LDS_THREADS) and nvec % 64
    print(f"[lds {IO_IDS[dtype]}] {cus()} CUs, [{rows}, {cols}]: {nvec} vectors, {-(-nvec // (cus() * LDS_THREADS))} trips, {nvec % 64} lanes in the last wave")
    xp, _ = recipe(PERIOD, cols // bs, bs, dtype, seed=11, alone=(2.0 ** -122, 2.0 ** -128, 2.0 ** -140))       # flushed at qe = 8 | 4 and 2 | fp32
    x = tile_rows(xp, rows)
    for name in (("fp8_e4m3", "fp6_e3m2", "fp4_e2m1") if pow2 else ("fp8_e4m3",)):
        host, fmt, lut = form_of(nv, name, "table")
        assert lut.data_ptr() % 16 == 0
        qmax = qmax_for(name)
        s_ref, q_ref = cpu_pair(xp, -1, bs, host, qmax, pow2)
        s_want, q_want = tile_rows(bits_of(s_ref), rows), tile_rows(bits_of(q_ref), rows)
        if name == "fp8_e4m3":
            got = c_quantize(nv, x, bs, fmt, lut, qmax, pow2, what=f"LDS table {name}")
            assert_same(got["s"], s_want, "scale")
            assert_same(got["q"], q_want, "q")
        if pow2:
            codes, e8, keep, _, nflush = pack_expectation(s_ref, q_ref, name, bs)
            assert nflush >= 1
            keep = tile_rows(keep, rows)
            got = c_quantize(nv, x, bs, fmt, lut, qmax, True, pack=name, what=f"LDS table, pack {name}")
            assert_same(got["s"], s_want, f"scale, pack {name}")
            assert_same(got["q"], q_want, f"q, pack {name}")
            assert_same(got["codes"][keep], tile_rows(codes, rows)[keep], f"codes {name}")
            assert_same(got["e8"][keep], tile_rows(e8, rows)[keep], f"e8m0 {name}")


# ---- c. the second grid-stride trip of the 256-thread variants ---------------------------------------------------------------------------
def second_trip_rows(group):
    """one block per row: rows whose vectors fill WG_PER_CU CU workgroups of 256 once, then three more workgroups and one block"""
    nvec = WG_PER_CU * cus() * 256 + 3 * 256 + group
    print(f"[second trip] {cus()} CUs, {nvec} vectors = {WG_PER_CU * cus()} workgroups of 256 + {3 * 256 + group}")
    return nvec // group


@pytest.mark.parametrize("variant", ["rows-pack", "misaligned", "closed"])
def test_second_trip_quantize(nv, variant):
    dtype, bs = BF16, 32
    group = bs // KPER[dtype]
    rows = second_trip_rows(group)
    if variant == "rows-pack":
        name, kind, pack = "fp8_e4m3", ("rows" if has_row_form("fp8_e4m3") else "misaligned"), "fp8_e4m3"
    else:
        name, kind, pack = ("fp8_e4m3", "misaligned", None) if variant == "misaligned" else ("int8", "closed", None)
    host, fmt, lut = form_of(nv, name, kind)
    qmax = qmax_for(name)
    xp, _ = recipe(PERIOD, 1, bs, dtype, seed=12, alone=(2.0 ** -122,))
    s_ref, q_ref = cpu_pair(xp, -1, bs, host, qmax, True)
    got = c_quantize(nv, tile_rows(xp, rows), bs, fmt, lut, qmax, True, pack=pack, what=f"second trip, {variant} ({kind})")
    assert_same(got["s"], tile_rows(bits_of(s_ref), rows), "scale")
    assert_same(got["q"], tile_rows(bits_of(q_ref), rows), "q")
    if pack:
        codes, e8, keep, _, nflush = pack_expectation(s_ref, q_ref, name, bs)
        assert nflush >= 1
        keep = tile_rows(keep, rows)
        assert_same(got["codes"][keep], tile_rows(codes, rows)[keep], "codes")
        assert_same(got["e8"][keep], tile_rows(e8, rows)[keep], "e8m0")


@pytest.mark.parametrize("form,dtype", [(("int8", "closed"), F32), (("fp8_e4m3", "table"), BF16), (("e4m3", "closed"), BF16), ((None, "identity"), BF16)],
                         ids=["int8-closed-f32", "fp8_e4m3-table-bf16", "e4m3-closed-bf16", "identity-bf16"])
def test_second_trip_fake_quant(nv, form, dtype):
    bs = 32
    rows = second_trip_rows(bs // KPER[dtype])
    _, fmt, lut = form_of(nv, *form)
    qmax = qmax_for(form[0])
    xp, _ = recipe(PERIOD, 1, bs, dtype, seed=13, alone=sweep_alone(dtype))
    y_ref, s_ref = oracle_fake_quant(xp, -1, bs, form[0], qmax, False)
    got = c_fake_quant(nv, tile_rows(xp, rows), bs, fmt, lut, qmax, what=f"second trip {form}")
    assert_same(got["s"], tile_rows(s_ref, rows), "scale")
    assert_same(got["y"], tile_rows(y_ref, rows), "y")


# ---- d. the packed operand ----------------------------------------------------------------------------------------------------------------
def pack_shapes(dtype):
    """(K, block size): K = 160 and 192 leave a row's code bytes off a power of two; blocks of 64 .. 64 kPer repeat their E8M0 byte"""
    return [(64, 32), (160, 32), (192, 32), (192, 64), (256, 128), (2 * 64 * KPER[dtype], 64 * KPER[dtype])]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
@pytest.mark.parametrize("name", sorted(BITS))
def test_pack_equals_the_host_packer(nv, name, dtype):
    qmax = qmax_of(name)
    qe = int(np.floor(np.log2(qmax)))
    kinds = ["table"] + (["rows"] if has_row_form(name) else []) + (["closed"] if name == "fp8_e4m3" else [])
    print(f"[pack {name} {IO_IDS[dtype]}] element passes: {kinds}")
    nrows, seen_flush, left, total = 12, 0, 0, 0
    for K, bs in pack_shapes(dtype):
        # a block whose amax gives the scale 2^-130 (below E8M0's 2^-127), and 2^-140 (fp32 only: bf16 has no such value)
        x, nonfinite = recipe(nrows, K // bs, bs, dtype, seed=K + bs, alone=(2.0 ** (qe - 130), 2.0 ** -140))
        for kind in kinds:
            host, fmt, lut = form_of(nv, "e4m3" if kind == "closed" else name, kind)
            s_ref, q_ref = cpu_pair(x, -1, bs, host, qmax, True)
            codes, e8, keep, values, nflush = pack_expectation(s_ref, q_ref, name, bs)
            left_out = nrows - int(keep.sum())
            assert left_out <= len(nonfinite), f"K={K} bs={bs}: {left_out} of {nrows} rows left out, {len(nonfinite)} hold a planted Inf / NaN"
            if kind == "table":
                seen_flush, left, total = seen_flush + nflush, left + left_out, total + nrows
            finite = np.isfinite(values) & ~keep[:, None]
            for want_q in (True, False):
                what = f"K={K} bs={bs} {kind} q={want_q}"
                got = c_quantize(nv, x, bs, fmt, lut, qmax, True, pack=name, want_q=want_q, what=what)
                assert_same(got["s"], bits_of(s_ref), f"scale {what}")
                if want_q:
                    assert_same(got["q"], bits_of(q_ref), f"q {what}")
                assert_same(got["codes"][keep], codes[keep], f"codes {what}")
                assert_same(got["e8"][keep], e8[keep], f"e8m0 {what}")
                # a row that holds an Inf or a NaN: every finite element of it still carries exactly its own code
                each = unpack_codes(got["codes"], BITS[name])
                assert each.shape == values.shape
                assert_same(each[finite], o.mx_encode(values[finite], name), f"codes of the finite elements of the rows left out, {what}")
    print(f"[pack {name} {IO_IDS[dtype]}] {left} of {total} code rows ({left / total:.2%}) left out of the row comparison (each holds a planted "
          f"Inf / NaN; their finite elements are compared code by code); {seen_flush} blocks flushed")
    assert seen_flush >= 1, "no block was flushed: the plant did not reach the rule"


# ---- e. every fp32 binade -------------------------------------------------------------------------------------------------------------------
def test_every_f32_binade(nv):
    """quant_max = 1 keeps every exponent observable: scale = 2^floor(log2(amax)) with torch's fp32 logarithm, which reaches the next
    integer from the thresholds of kMxLog2ThrF32 on; the subnormal patterns take the __clz branch of floor_log2_dtype.  One block of 4
    per pattern, the pattern in lane element i % 4, the rest of the block zero.  (tests/test_mx_log2_tables_cpu.py checks the table
    itself against this machine's torch at the same patterns.)"""
    host, fmt, lut = form_of(nv, "fp8_e4m3", "table")
    normal, sub = f32_binade_patterns()
    pats = np.concatenate([normal, sub])
    xb = np.zeros((len(pats), 4), np.uint32)
    xb[np.arange(len(pats)), np.arange(len(pats)) % 4] = pats
    x = torch.from_numpy(xb.view(np.int32)).view(F32)
    s_ref, q_ref = cpu_pair(x, -1, 4, host, 1.0, True)
    got = c_quantize(nv, x, 4, fmt, lut, 1.0, True, what="every binade")
    assert_same(got["s"], bits_of(s_ref), "scale")
    assert_same(got["q"], bits_of(q_ref), "q")


# ---- f. the scale map through the C ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=IO_IDS.get)
def test_scale_map(nv, dtype):
    host, fmt, lut = form_of(nv, "fp4_e2m1", "table")
    shost, _, sdev = form_of(nv, "fp8_e4m3", "table")
    for rows, nblk in ((3, 5), (3, 43 * 4 * KPER[dtype] // 16)):                 # the second: 516 vectors
        x, _ = recipe(rows, nblk, 16, dtype, seed=2)
        s_ref, q_ref = cpu_pair(x, -1, 16, host, 6.0, False, shost)
        got = c_quantize(nv, x, 16, fmt, lut, 6.0, False, smap=sdev, what="scale map")
        assert_same(got["s"], bits_of(s_ref), "scale")
        assert_same(got["q"], bits_of(q_ref), "q")
        y_ref, s_ref = oracle_fake_quant(x, -1, 16, "fp4_e2m1", 6.0, False, "fp8_e4m3")
        got = c_fake_quant(nv, x, 16, fmt, lut, 6.0, smap=sdev, what="scale map, fake-quant")
        assert_same(got["s"], s_ref, "scale (fake-quant)")
        assert_same(got["y"], y_ref, "y")


# ---- g. through the operator at the size where the plain table moves to LDS ------------------------------------------------------------
def test_operator_at_the_lds_size(nv):
    from quantized_training import mx_operand
    from quantized_training.fake_quantize import get_quantization_map
    host, qmap = get_quantization_map("fp8_e4m3", "cpu"), get_quantization_map("fp8_e4m3", "cuda")
    cols, bs = 512, 32
    rows = -(-max(LDS_MIN, cus() * LDS_THREADS * 8) // cols) + 3
    assert rows * cols >= LDS_MIN
    xp, _ = recipe(PERIOD, cols // bs, bs, BF16, seed=14, alone=(2.0 ** -122,))
    s_ref, q_ref = cpu_pair(xp, -1, bs, host, 448.0, True)
    s, q = torch.ops.quantized_ops.quantize_mx(tile_rows(xp, rows).cuda(), qmap, [-1], bs, 448.0, True, None, None)
    assert_same(bits_of(s), tile_rows(bits_of(s_ref), rows), "scale")
    assert_same(bits_of(q), tile_rows(bits_of(q_ref), rows), "q")
    fid, rbs, codes, e8 = mx_operand.operand_record(q, mx_operand.ROWS)
    assert (fid, rbs, tuple(codes.shape), tuple(e8.shape)) == (0, bs, (rows, cols), (rows, cols // 32))
    want_codes, want_e8, keep, _, nflush = pack_expectation(s_ref, q_ref, "fp8_e4m3", bs)
    assert nflush >= 1
    keep = tile_rows(keep, rows)
    assert_same(codes.cpu().numpy()[keep], tile_rows(want_codes, rows)[keep], "codes")
    assert_same(e8.cpu().numpy()[keep], tile_rows(want_e8, rows)[keep], "e8m0")


# ---- h. refusals: nothing is written ------------------------------------------------------------------------------------------------------
BAD_ARG, UNALIGNED = "QT_ERR_BAD_ARG", "QT_ERR_UNALIGNED"


def declines(kper):
    """every decline of launch (csrc/qt_mx_quant.hip) and launch_mx (csrc/qt_elementwise.hip) as overrides of a call that would be taken"""
    both = {
        "NULL x": (dict(x="null"), BAD_ARG), "NULL scales": (dict(s="null"), BAD_ARG), "NULL fmt": (dict(fmt=False), BAD_ARG),
        "table format without a table": (dict(lut=False), BAD_ARG),
        "block size 0": (dict(bs=0), BAD_ARG), "block size below a vector": (dict(bs=kper // 2), BAD_ARG),
        "block size 48": (dict(bs=48, cols=96), BAD_ARG), "block size above 64 vectors": (dict(bs=128 * kper, cols=128 * kper), BAD_ARG),
        "cols % block_size": (dict(cols=72), UNALIGNED), "x off 16 bytes": (dict(x="off"), UNALIGNED), "q / y off 16 bytes": (dict(q="off"), UNALIGNED),
    }
    quantize = {"quant_max 0": (dict(qmax=0.0), BAD_ARG), "quant_max negative": (dict(qmax=-1.0), BAD_ARG),
                "quant_max NaN": (dict(qmax=float("nan")), BAD_ARG)}
    pack = {"codes without e8m0": (dict(e8="null"), BAD_ARG), "e8m0 without codes": (dict(codes="null"), BAD_ARG),
            "pack without force_pow2": (dict(pow2=0), BAD_ARG), "pack_format 5": (dict(pf=5), BAD_ARG), "pack_format -1": (dict(pf=-1), BAD_ARG),
            "pack with block size 16": (dict(bs=16), BAD_ARG)}
    return both, quantize, pack


@pytest.mark.parametrize("io", ["bf16", "f32"])
def test_refusals_write_nothing(nv, io):
    _, fmt, devm = form_of(nv, "fp8_e4m3", "table")
    L = nv.lib()
    kper = 8 if io == "bf16" else 4
    npdt = np.uint16 if io == "bf16" else np.uint32
    # every buffer holds the largest tensor any override describes (2 x 128 kPer), so a call that were taken by mistake stays in bounds
    big = 128 * kper
    x = torch.randn(2 * big + 64, device="cuda").to(BF16 if io == "bf16" else F32)
    full = {"q": ((2, big), npdt), "s": ((2, big), npdt), "codes": ((2, big), np.uint8), "e8": ((2, big), np.uint8)}
    both, quantize, pack = declines(kper)

    def pointer(base, mode):
        return {"ok": base, "null": None, "off": base + 8}[mode]

    def call_of(family, want, **kw):
        a = dict(x="ok", q="ok", s="ok", codes="ok", e8="ok", rows=2, cols=64, bs=32, fmt=True, lut=True, qmax=448.0, pow2=1, pf=0)
        a.update(kw)
        F, lut = (ctypes.byref(fmt) if a["fmt"] else None), (devm.data_ptr() if a["lut"] else None)

        def call(outs):
            xp, qp, sp = pointer(x.data_ptr(), a["x"]), pointer(outs["q"].ptr, a["q"]), pointer(outs["s"].ptr, a["s"])
            if family == "quantize":
                rc = getattr(L, "qt_quantize_mx_" + io)(xp, qp, sp, pointer(outs["codes"].ptr, a["codes"]), pointer(outs["e8"].ptr, a["e8"]),
                                                        a["rows"], a["cols"], a["bs"], F, lut, a["qmax"], a["pow2"], None, a["pf"], stream())
            else:
                rc = getattr(L, "qt_fake_quant_mx_" + io)(xp, qp, sp, a["rows"], a["cols"], a["bs"], F, lut, a["qmax"], None, stream())
            assert want is None or rc == getattr(nv, want), f"status {rc}, expected {want}"
            return rc
        return call

    for what, (kw, want) in {**both, **quantize, **pack}.items():
        refused(call_of("quantize", want, **kw), full, f"quantize_{io}: {what}")
    for what, (kw, want) in {**both, **quantize}.items():                      # without a pack the same declines hold
        refused(call_of("quantize", want, codes="null", e8="null", **kw), full, f"quantize_{io}, no pack: {what}")
    for what, (kw, want) in {**both, "NULL y": (dict(q="null"), BAD_ARG)}.items():
        refused(call_of("fake_quant", want, **kw), {"q": full["q"], "s": full["s"]}, f"fake_quant_{io}: {what}")
    # an empty tensor: QT_OK and nothing written, whatever else the call says
    for family in ("quantize", "fake_quant"):
        for kw in (dict(rows=0), dict(cols=0), dict(rows=0, x="null", q="null", s="null")):
            outs = {k: Guarded(*v) for k, v in full.items()}
            assert call_of(family, None, **kw)(outs) == 0, f"{family}_{io}: empty tensor {kw}"
            torch.cuda.synchronize()
            assert all(g.untouched() for g in outs.values()), f"{family}_{io}: an empty tensor wrote something"
