"""The per-channel fake-quantizer qt_fake_quant_pc_bf16 / qt_fake_quant_pc_f32 (csrc/qt_elementwise.hip, launch_pc_kind) on every launch
route, called through the C ABI, bit for bit against the numpy oracle (NaNs canonicalised; no tolerance anywhere).

x is viewed [outer][C][inner], rows = outer * C, kPer = 8 (bf16) / 4 (fp32) elements per 16-byte vector, CU = compute units of the
device, R = 16 * CU + 37 rows -- past the row cap of the vec, scalar and LDS-table kernels (their grids stop at 16 * CU rows per pass),
and no multiple of anything.  `route()` below restates launch_pc_kind's choice and every launch asserts the route it expects.

  case                                                                  route     kernel
  --------------------------------------------------------------------  --------  -------------------------------------------------
  test_vec_route         inner = 64 kPer, 65 kPer; rows >= R            vec       fq_pc_vec_kernel<IO, KIND>  (plain table: n < 2^21)
  test_lds_table_route   plain table, n >= 2^21; rows >= R, 16 CU - 3   vec-lds   fq_pc_vec_lds_kernel (1024 threads, a wave per row)
  test_row_form_route    p1 & 1, 256- and 512-row tables; rows >= R     vec-rows  fq_pc_vec_kernel<IO, kFmtRows>
  test_scalar_route      inner = 7, 24, 100, 63 kPer, 64 kPer + 1       scalar    fq_pc_kernel
  test_misaligned_...    inner = 64 kPer, x or y 2 / 4 bytes off        scalar    fq_pc_kernel (equals the aligned vec launch)
  test_last_route        inner = 1; C = 1, 7, 40; n > 8 CU 256          last      fq_pc_last_kernel
  test_every_bf16_pattern / test_f32_patterns_with_low_halves           vec, vec-rows, scalar, last; fp32 plain table (2^21): vec-lds
  test_observe_only_and_no_observer_forms    y = NULL | amax = NULL     last, vec, scalar
  test_rows_equal_the_per_tensor_launch      ~50 rows                   vec, scalar  (against qt_fake_quant_bf16 / _f32 row by row)

Scales: channel c takes SCALES[c % 5] -- 1 (kDivUnit), a power of two and two other values (kDivFast and its redo), 2^-110 (outside
UniformDiv's band, kDivExact) -- so neighbouring rows of one launch take different division paths.  The amax slots start as a mix of
zero, a value below and a value above the channel's maximum; y starts as NaN everywhere, with eight guard elements on both sides that
must still be NaN afterwards, so a row the kernel skipped fails the comparison instead of matching stale memory."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

QT_OK, QT_ERR_BAD_ARG = 0, -2
LUT_FMT = (0, 0, 0, 0.0, 0.0)                      # QT_FMT_LUT without the row bit: the map as a plain table
LDS_MIN = 1 << 21                                  # csrc kLutLdsMinElems
GUARD = 8                                          # elements on each side of every device buffer of this module


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Io:
    """One tensor dtype of the entry point; tensors travel as their bit patterns (uint16 / uint32), so NaN payloads survive."""

    def __init__(self, name, k_per, bits, pc, per_tensor):
        self.name, self.k_per, self.bits, self.pc, self.per_tensor = name, k_per, bits, pc, per_tensor
        self.bf16 = name == "bf16"
        self.signed = np.int16 if self.bf16 else np.int32
        self.torch = torch.int16 if self.bf16 else torch.int32
        self.esz = 2 if self.bf16 else 4
        self.nan = 0x7FC0 if self.bf16 else 0x7FC00000

    def __repr__(self):
        return self.name

    def from_f32(self, x):
        return o.f32_to_bf16(x).reshape(x.shape) if self.bf16 else np.ascontiguousarray(x, np.float32).view(np.uint32)

    def canon(self, b):
        return o.canon_nan16(b) if self.bf16 else o.canon_nan32(b)

    def magnitude(self, b):
        """What the observer max-accumulates: the fp32 image of |x| as an unsigned integer (a NaN wins, like torch.amax)."""
        return ((b & 0x7FFF).astype(np.uint32) << 16) if self.bf16 else (b & np.uint32(0x7FFFFFFF))


BF16 = Io("bf16", 8, np.uint16, "qt_fake_quant_pc_bf16", "qt_fake_quant_bf16")
F32 = Io("f32", 4, np.uint32, "qt_fake_quant_pc_f32", "qt_fake_quant_f32")
IOS = [BF16, F32]

SCALES = (1.0, 0.25, 0.037, 3.5, 2.0 ** -110)      # unit | fast: power of two, two others | exact (2^-110 is a bf16 and an fp32 value)
FORMATS = ["int8", "e4m3", "posit8_1-table", "identity"]


def channel_scales(C, pool=SCALES):
    return np.asarray(pool, np.float32)[np.arange(C) % len(pool)]


# ---- formats ---------------------------------------------------------------------------------------------------------
_FORMATS = {}


def launch_format(nv, key):
    """(qt_format, device map, the oracle's map) of FORMATS / of "<dtype>-rows", the row form as the product launches a table format."""
    if key not in _FORMATS:
        dtype, _, how = key.partition("-")
        if key == "identity":
            fmt, lut, qmap = nv.format_for(None), nv.build_map_u16(None), o.get_quantization_map(None)
            assert fmt.kind == nv.QT_FMT_IDENTITY
        elif how == "rows":
            import quantized_training as qt
            from quantized_training.fake_quantize import _launch_format
            lut = qt.get_quantization_map(dtype, torch.device("cuda", torch.cuda.current_device()))
            base = nv.format_for(dtype)
            fmt = _launch_format(base if base.kind == nv.QT_FMT_LUT else nv.QtFormat(*LUT_FMT), lut)
            assert fmt.kind == nv.QT_FMT_LUT and (fmt.p1 & 1), (dtype, "the row form covers this map")
            qmap = o.get_quantization_map(dtype)
        else:
            fmt = nv.QtFormat(*LUT_FMT) if how == "table" else nv.format_for(dtype)
            assert fmt.kind == {"int8": nv.QT_FMT_INT, "e4m3": nv.QT_FMT_FP_SAT}.get(key, nv.QT_FMT_LUT), key
            lut, qmap = nv.build_map_u16(dtype), o.get_quantization_map(dtype)
        if isinstance(lut, np.ndarray):
            lut = torch.from_numpy(lut.view(np.int16)).cuda()
        _FORMATS[key] = (fmt, lut, qmap)
    return _FORMATS[key]


# ---- sizes and routes ------------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def row_cap():
    return 16 * cu_count()                         # grid_for(rows, 1, 16) blocks of one row; grid_for(rows, 16, 1) blocks of 16 waves


def past_cap():
    return row_cap() + 37                          # R


def three_by(rows):
    """(outer, C) = (3, ceil(rows / 3)): at least `rows` rows, three rows per channel that meet in one amax slot."""
    return 3, -(-rows // 3)


def route(nv, io, fmt, outer, C, inner, x_ptr, y_ptr):
    """launch_pc_kind's choice, restated."""
    if inner == 1:
        return "last"
    if inner % io.k_per == 0 and inner >= 64 * io.k_per and x_ptr % 16 == 0 and (y_ptr or 0) % 16 == 0:
        if fmt.kind == nv.QT_FMT_LUT and (fmt.p1 & 1) and y_ptr:
            return "vec-rows"
        if fmt.kind == nv.QT_FMT_LUT and y_ptr and outer * C * inner >= LDS_MIN:
            return "vec-lds"
        return "vec"
    return "scalar"


# ---- data, expectations ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=3)
def random_data(io, outer, C, inner):
    """randn times a per-channel magnitude spanning 2^-6 .. 2^6, as bit patterns [outer, C, inner] (shared: do not write to it)."""
    rng = np.random.default_rng(outer * 1000003 + C * 1009 + inner)
    mag = (2.0 ** rng.uniform(-6, 6, (1, C, 1))).astype(np.float32)
    x = io.from_f32(rng.standard_normal((outer, C, inner), dtype=np.float32) * mag)
    x.setflags(write=False)
    return x


SPECIALS = np.array([0x7FC0, 0xFFC1, 0x7F80, 0xFF80, 0x0000, 0x8000, 0x0001, 0x807F, 0x0080, 0x7F7F, 0xFF7F, 0x3F80], np.uint16)


def salted(io, x):
    """`x` with NaN, +-Inf, +-0, subnormals and the largest finite values at the head of every row."""
    x = x.copy()
    sp = SPECIALS if io.bf16 else (SPECIALS.astype(np.uint32) << 16) | np.uint32(1)
    if not io.bf16:
        sp[2:6] &= np.uint32(0xFFFF0000)           # keep the infinities and zeros what they are
    x[:, :, :sp.size] = sp
    return x


def expect_y(io, x, qmap, scales):
    """The oracle's fake-quant of bit patterns x [outer, C, inner] with scale[c]; bf16 tensors see the scale rounded to bf16."""
    s = np.asarray(scales, np.float32).reshape(1, -1, 1)
    if io.bf16:
        return o.canon_nan16(o.fq_bf16(x, qmap, o.f32_to_bf16(s).reshape(s.shape)))
    return o.canon_nan32(o.fq_f32(x.view(np.float32), qmap, s).view(np.uint32))


def channel_max(io, x):
    return io.magnitude(x).max(axis=(0, 2)).astype(np.uint32)


def mixed_start(cmax):
    """Slot contents before the launch: zero, a value below the channel's maximum, a value above it, in turn."""
    below = cmax >> 1
    above = np.minimum(cmax.astype(np.uint64) + 0x00800000, 0x7FFFFFFF).astype(np.uint32)
    return np.choose(np.arange(cmax.size) % 3, [np.zeros_like(cmax), below, above]).astype(np.uint32)


def expect_amax(io, x, start):
    return np.maximum(channel_max(io, x), start)


# ---- launches --------------------------------------------------------------------------------------------------------
def device_bits(io, bits, off=0):
    """`bits` copied `off` elements into an allocation of its own."""
    a = np.ascontiguousarray(bits).reshape(-1)
    buf = torch.empty(a.size + 2 * GUARD, dtype=io.torch, device="cuda")
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(a.view(io.signed).copy()))
    return view


def run_pc(nv, io, x, key, scales, start, want, y=True, x_off=0, y_off=0):
    """One qt_fake_quant_pc_* launch on bit patterns x [outer, C, inner] -> (canonical output bits like x | None, amax slots | None).
    start: the slots' contents before the launch (None: no observer).  y = False: observe only.  `want`: the route it must take."""
    fmt, lut, _ = launch_format(nv, key)
    outer, C, inner = x.shape
    xd = device_bits(io, x, x_off)
    nan = int(np.array([io.nan], io.bits).view(io.signed)[0])
    ybuf = torch.full((x.size + 2 * GUARD,), nan, dtype=io.torch, device="cuda") if y else None
    yd = ybuf[GUARD + y_off:GUARD + y_off + x.size] if y else None
    sd = torch.from_numpy(np.ascontiguousarray(scales, np.float32)).cuda()
    ad = torch.from_numpy(np.ascontiguousarray(start, np.uint32).view(np.int32).copy()).cuda() if start is not None else None
    assert sd.numel() == C and (ad is None or ad.numel() == C)
    assert xd.data_ptr() % 16 == (x_off * io.esz) % 16 and (yd is None or yd.data_ptr() % 16 == ((GUARD + y_off) * io.esz) % 16)
    got = route(nv, io, fmt, outer, C, inner, xd.data_ptr(), yd.data_ptr() if y else None)
    assert got == want, (got, want, io, key, x.shape)
    nv.check(getattr(nv.lib(), io.pc)(xd.data_ptr(), yd.data_ptr() if y else None, outer, C, inner, ctypes.byref(fmt), lut.data_ptr(),
                                     sd.data_ptr(), ad.data_ptr() if ad is not None else None, stream()), io.pc)
    torch.cuda.synchronize()
    out = None
    if y:
        whole = ybuf.cpu().numpy().view(io.bits)
        lo = GUARD + y_off
        assert np.all(whole[:lo] == io.nan) and np.all(whole[lo + x.size:] == io.nan), "wrote outside y"
        out = io.canon(whole[lo:lo + x.size]).reshape(x.shape)
    return out, (ad.cpu().numpy().view(np.uint32) if ad is not None else None)


def check_case(nv, io, key, x, want, **kw):
    """Full launch (output and observer, mixed slot contents) on `x` against the oracle."""
    C = x.shape[1]
    scales = channel_scales(C)
    start = mixed_start(channel_max(io, x))
    y, amax = run_pc(nv, io, x, key, scales, start, want, **kw)
    exp = expect_y(io, x, launch_format(nv, key)[2], scales)
    bad = np.flatnonzero((y != exp).reshape(-1))
    assert bad.size == 0, (io, key, x.shape, "first mismatches at", bad[:8].tolist(), "rows", (bad[:8] // x.shape[2]).tolist())
    assert np.array_equal(amax, expect_amax(io, x, start)), (io, key, x.shape)
    return y, amax


# ---- 1. every route, past its grid cap, ragged channel counts ----------------------------------------------------------
@pytest.mark.parametrize("vecs", [64, 65])                      # 64: the smallest inner that qualifies; 65: the last 256-lane pass is ragged
@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_vec_route(nv, io, key, vecs):
    """fq_pc_vec_kernel with more rows than its grid takes in one pass.  A plain bf16 table with an output cannot be there: rows past
    the cap times 64 vectors are 2^21 elements, the LDS-table kernel's; it gets the most rows that stay below (the gather kernel past
    its cap with a plain table: fp32 here, and the observe-only launch of test_observe_only_and_no_observer_forms)."""
    inner = vecs * io.k_per
    outer, C = three_by(past_cap())
    if key.endswith("-table") and outer * C * inner >= LDS_MIN:
        # a plain table stays on the gather kernel below 2^21 elements only: 4093 rows of 512 bf16 elements are 2 095 616 of them
        outer, C = 1, min(4093, (LDS_MIN - 1) // inner)
        assert outer * C * inner < LDS_MIN and (inner != 512 or outer * C * inner == 2095616)
    else:
        assert outer * C > row_cap()                              # the row loop runs a second time
    check_case(nv, io, key, random_data(io, outer, C, inner), "vec")


@pytest.mark.parametrize("rows", ["past the cap", "idle waves"])
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_lds_table_route(nv, io, rows):
    """fq_pc_vec_lds_kernel, one wave per row: more rows than waves in the grid (some waves take two rows, most one), and three rows
    fewer than waves (the last workgroup has idle waves).  NaN, Inf, zeros and subnormals sit at the head of every row."""
    if rows == "past the cap":
        (outer, C), inner = three_by(past_cap()), (64 if io.bf16 else 128) * io.k_per
        assert outer * C > row_cap() and (outer * C) % 16 != 0
    else:
        (outer, C), inner = (1, row_cap() - 3), (65 if io.bf16 else 130) * io.k_per
        assert -(-outer * C // 16) * 16 - outer * C == 3
    assert outer * C * inner >= LDS_MIN
    check_case(nv, io, "posit8_1-table", salted(io, random_data(io, outer, C, inner)), "vec-lds")


def test_row_form_tables_have_both_sizes(nv):
    assert not (launch_format(nv, "posit8_1-rows")[0].p1 & 2) and (launch_format(nv, "int4-rows")[0].p1 & 2)   # 256 and 512 row words


@pytest.mark.parametrize("dtype", ["posit8_1", "int4"])         # 256 and 512 row words in LDS
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_row_form_route(nv, io, dtype):
    """The row form equals the oracle, and equals the same map launched as a plain table on the same data."""
    (outer, C), inner = three_by(past_cap()), 64 * io.k_per
    assert outer * C > row_cap()
    x = salted(io, random_data(io, outer, C, inner))
    y, amax = check_case(nv, io, dtype + "-rows", x, "vec-rows")
    fmt, lut, qmap = launch_format(nv, dtype + "-rows")
    _FORMATS[dtype + "-same map, plain"] = (nv.QtFormat(*LUT_FMT), lut, qmap)
    plain = "vec-lds" if x.size >= LDS_MIN else "vec"
    y2, amax2 = run_pc(nv, io, x, dtype + "-same map, plain", channel_scales(C), mixed_start(channel_max(io, x)), plain)
    assert np.array_equal(y, y2) and np.array_equal(amax, amax2)


@pytest.mark.parametrize("inner_of", [lambda k: 7, lambda k: 24, lambda k: 100, lambda k: 64 * k - k, lambda k: 64 * k + 1],
                         ids=["7", "24", "100", "63kPer", "64kPer+1"])
@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_scalar_route(nv, io, key, inner_of):
    """Short rows (7, 24, 100, 63 vectors) and a long ragged one: fq_pc_kernel, its row loop in a second pass."""
    inner = inner_of(io.k_per)
    assert inner % io.k_per != 0 or inner < 64 * io.k_per
    outer, C = three_by(past_cap())
    assert outer * C > row_cap()
    check_case(nv, io, key, random_data(io, outer, C, inner), "scalar")


@pytest.mark.parametrize("which", ["x", "y"])
@pytest.mark.parametrize("key", FORMATS)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_misaligned_pointer_takes_the_scalar_route(nv, io, key, which):
    """Rows the vec route would take, with x (or only y) one element into its allocation: the element-wise kernel, the same bits."""
    (outer, C), inner = three_by(past_cap()), 64 * io.k_per
    x = random_data(io, outer, C, inner)
    off = {which + "_off": 1}
    assert (1 * io.esz) % 16 != 0                                 # run_pc asserts data_ptr() % 16 == this
    y, amax = check_case(nv, io, key, x, "scalar", **off)
    aligned = "vec-lds" if (key.endswith("-table") and x.size >= LDS_MIN) else "vec"
    y2, amax2 = run_pc(nv, io, x, key, channel_scales(C), mixed_start(channel_max(io, x)), aligned)
    assert np.array_equal(y, y2) and np.array_equal(amax, amax2)


def last_shapes():
    per_pass = 8 * cu_count() * 256                               # grid_for(n, 1024, 8) blocks of 256 threads, one element each per pass
    outer7 = per_pass // 7 + 5102                                 # C = 7: n = 560 000 on a 256-CU part, the element loop runs twice
    assert outer7 * 7 > per_pass
    return {1: (1000, 1), 7: (outer7, 7), 40: (300, 40)}


@pytest.mark.parametrize("C", [1, 7, 40])
@pytest.mark.parametrize("key", FORMATS + ["posit8_1-rows"])      # (a table format's row bit is not used on this route: the plain gather)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_last_route(nv, io, key, C):
    outer, C = last_shapes()[C]
    check_case(nv, io, key, random_data(io, outer, C, 1), "last")


# ---- 2. every bf16 pattern through every per-row path -----------------------------------------------------------------
def _many_scales():
    """24 scales: those of test_gpu_parity.test_division_by_many_scales (its fixed ones and its first nine drawn ones) and 1, 2^-110, 2^100."""
    rng = np.random.default_rng(42)
    drawn = list(2.0 ** rng.uniform(-24, 19, 24))[:9]
    fixed = [2.0 ** -25, 2.0 ** 20, 2.0 ** -30, 2.0 ** 40, 1e-38, 3e38, 0.1, 1.0 / 3.0, 448.0, 1.0 / 448.0, 127.0, 5e-7]
    return tuple(float(np.float32(s)) for s in drawn + fixed + [1.0, 2.0 ** -110, 2.0 ** 100])


SCALES_24 = _many_scales()
SCALES_8 = tuple(float(np.float32(s)) for s in (1.0, 0.037, 3.5, 1.0 / 3.0, 0.1, 448.0, 2.0 ** -110, 2.0 ** 100))
assert len(SCALES_24) == 24 and len(set(SCALES_24)) == 24


def bf16_patterns(finite):
    p = o.all_bf16_patterns()
    if finite:
        p = p[(p & 0x7FFF) < 0x7F80]
        p = np.concatenate([p, np.zeros(-p.size % 8, np.uint16)])                  # whole 16-byte vectors
    return p


def f32_patterns(finite):
    """The bf16 patterns widened, and each with a low half of 0x0001, 0x8000 and 0xFFFF: the fold hi16 | (lo16 != 0), fast32's redo."""
    hi = bf16_patterns(finite).astype(np.uint32) << 16
    return np.concatenate([hi] + [hi | np.uint32(low) for low in (1, 0x8000, 0xFFFF)])


def layouts(io, p, pool):
    """The three views of `p` repeated once per scale -> {route: (x [outer, C, inner], scale[c])}."""
    S = len(pool)
    rows = np.tile(p, (S, 1))
    return {"vec": (rows.reshape(1, S, p.size), channel_scales(S, pool)),
            "scalar": (rows.reshape(1, S * p.size // 8, 8), channel_scales(S * p.size // 8, pool)),
            "last": (np.ascontiguousarray(rows.T).reshape(p.size, S, 1), channel_scales(S, pool))}


def check_patterns(nv, io, p, pool, key, finite):
    for want, (x, scales) in layouts(io, p, pool).items():
        outer, C, inner = x.shape
        assert {"vec": inner >= 64 * io.k_per and inner % io.k_per == 0, "scalar": 1 < inner < 64 * io.k_per, "last": inner == 1}[want]
        if want == "vec" and key.endswith("-rows"):
            want = "vec-rows"
        if want == "vec" and key.endswith("-table") and x.size >= LDS_MIN:         # fp32, all patterns: 8 * 4 * 65 536 = 2^21 exactly
            want = "vec-lds"
        cmax = channel_max(io, x)
        start = mixed_start(cmax)
        y, amax = run_pc(nv, io, x, key, scales, start, want)
        exp = expect_y(io, x, launch_format(nv, key)[2], scales)
        bad = np.flatnonzero((y != exp).reshape(-1))
        assert bad.size == 0, (io, key, want, "first mismatches at", bad[:8].tolist())
        assert np.array_equal(amax, np.maximum(cmax, start)), (io, key, want)
        if want != "scalar":                                                        # every channel holds every pattern
            top = 0x7F800000
            assert np.all(cmax < top) if finite else np.all(cmax > top), "finite maxima | every channel's amax is a NaN pattern"


@pytest.mark.parametrize("finite", [False, True], ids=["all", "finite"])
@pytest.mark.parametrize("key", ["e4m3", "int8", "posit8_1-table", "posit8_1-rows"])
def test_every_bf16_pattern(nv, key, finite):
    """All 65 536 bf16 inputs (then the finite ones alone, so that finite amax values are compared too) under 24 scales: as [24, 65 536]
    (vec), as [24 * 8192, 8] (scalar, short rows) and transposed as [65 536, 24] with inner = 1 (last)."""
    check_patterns(nv, BF16, bf16_patterns(finite), SCALES_24, key, finite)


@pytest.mark.parametrize("finite", [False, True], ids=["all", "finite"])
@pytest.mark.parametrize("key", ["e4m3", "int8", "posit8_1-table", "posit8_1-rows"])
def test_f32_patterns_with_low_halves(nv, key, finite):
    """fp32: the same patterns widened, each also with a non-zero low half (4 x 65 536 inputs), under eight scales.  With every pattern
    the tensor has exactly 2^21 elements, so the plain table is staged in LDS on the vec layout; the finite set stays on the gather."""
    check_patterns(nv, F32, f32_patterns(finite), SCALES_8, key, finite)


# ---- 3. observe-only and no-observer forms -----------------------------------------------------------------------------
@pytest.mark.parametrize("want", ["last", "vec", "scalar"])
@pytest.mark.parametrize("key", ["e4m3", "posit8_1-table"])
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_observe_only_and_no_observer_forms(nv, io, key, want):
    """y = NULL (the map pointer still given) leaves the amax slots of the full launch; amax = NULL writes the y of the full launch."""
    if want == "last":
        outer, C, inner = last_shapes()[7] + (1,)
    else:
        (outer, C), inner = three_by(past_cap()), {"vec": 64 * io.k_per, "scalar": 24}[want]
        assert outer * C > row_cap()
    # a plain table of 2^21 elements or more is staged in LDS when there is an output to write, and gathered from when only observing
    with_y = "vec-lds" if (want == "vec" and key.endswith("-table") and outer * C * inner >= LDS_MIN) else want
    x = random_data(io, outer, C, inner)
    scales = channel_scales(C)
    start = mixed_start(channel_max(io, x))
    y, amax = run_pc(nv, io, x, key, scales, start, with_y)
    assert np.array_equal(amax, expect_amax(io, x, start))
    none, amax_only = run_pc(nv, io, x, key, scales, start, want, y=False)
    assert none is None and np.array_equal(amax_only, amax)
    y_only, none = run_pc(nv, io, x, key, scales, None, with_y)
    assert none is None and np.array_equal(y_only, y)


@pytest.mark.parametrize("io", IOS, ids=repr)
def test_empty_and_outputless_calls(nv, io):
    fmt, lut, _ = launch_format(nv, "e4m3")
    fn = getattr(nv.lib(), io.pc)
    nan = int(np.array([io.nan], io.bits).view(io.signed)[0])
    x = device_bits(io, np.zeros(64, io.bits))
    y = torch.full((64,), nan, dtype=io.torch, device="cuda")
    amax = torch.full((4,), 5, dtype=torch.int32, device="cuda")
    sc = torch.ones(4, device="cuda")
    for outer, C, inner in ((0, 4, 16), (4, 0, 16), (1, 4, 0)):
        assert fn(x.data_ptr(), y.data_ptr(), outer, C, inner, ctypes.byref(fmt), lut.data_ptr(), sc.data_ptr(), amax.data_ptr(), stream()) == QT_OK
    assert fn(x.data_ptr(), None, 1, 4, 16, ctypes.byref(fmt), lut.data_ptr(), sc.data_ptr(), None, stream()) == QT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((y == nan).all()) and bool((amax == 5).all())


# ---- 4. per-channel equals per-tensor, row by row ----------------------------------------------------------------------
@pytest.mark.parametrize("want", ["vec", "scalar"])
@pytest.mark.parametrize("key", ["e4m3", "posit8_1-table"])
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_rows_equal_the_per_tensor_launch(nv, io, key, want):
    """Every row of a 50-row launch equals qt_fake_quant_bf16 / _f32 on that row alone with that row's scale, output and amax: the
    entry point the oracle covers exhaustively (tests/test_gpu_parity.py)."""
    outer, C, inner = 2, 25, {"vec": 64 * io.k_per, "scalar": 100}[want]
    x = salted(io, random_data(io, outer, C, inner))
    scales = channel_scales(C)
    y, amax = run_pc(nv, io, x, key, scales, np.zeros(C, np.uint32), want)
    fmt, lut, _ = launch_format(nv, key)
    xd = device_bits(io, x)
    yd = torch.zeros(x.size, dtype=io.torch, device="cuda")
    sd = torch.from_numpy(scales).cuda()
    ad = torch.zeros(outer * C, dtype=torch.int32, device="cuda")
    fn = getattr(nv.lib(), io.per_tensor)
    for row in range(outer * C):
        at = row * inner * io.esz
        nv.check(fn(xd.data_ptr() + at, yd.data_ptr() + at, inner, ctypes.byref(fmt), lut.data_ptr(), sd.data_ptr() + 4 * (row % C),
                    ad.data_ptr() + 4 * row, stream()), io.per_tensor)
    torch.cuda.synchronize()
    assert np.array_equal(y.reshape(-1), io.canon(yd.cpu().numpy().view(io.bits)))
    assert np.array_equal(amax, ad.cpu().numpy().view(np.uint32).reshape(outer, C).max(axis=0))
