"""The per-tensor fake-quantizers qt_fake_quant_bf16 / qt_fake_quant_f32 (csrc/qt_elementwise.hip, launch_fq_kind) and the strided-rows
pass qt_fake_quant_rows_bf16 on every launch route, called through the C ABI, bit for bit against the numpy oracle (NaNs canonicalised;
no tolerance anywhere).

kPer = 8 (bf16) / 4 (fp32) elements per 16-byte vector, nvec = n // kPer, SHORT = 256 * 8 * 256 * 2 vectors (csrc kRowsDirectMaxVecs),
CU = compute units of the device.  `route()` below restates launch_fq_kind's choice and every launch asserts the route it expects.

  case                         n                                      route (not observed | observed)        kernel
  ---------------------------  -------------------------------------  -------------------------------------  ---------------------------
  test_element_gather          4095; 9000 with x and y one element     gather                                 fq_gather_kernel
                               into their allocations
  test_short_closed_form       4096 + 8 + 3; kPer (2 * 1024 + 17) + 5  closed-256 | closed-1024               fq_kernel<IO, KIND, ., 256 | 1024>
  test_short_row_form (bf16)   the same two                           rows-global-256 | rows-global-1024     fq_kernel, row words in global memory
  test_short_plain_table       the same two (n < 2^21)                table-global                           fq_kernel, map in global memory
  test_plain_table_in_lds      2^21 + 8 * 1024 * 5 + 3                table-lds                              fq_kernel<IO, QT_FMT_LUT, ., 1024, 4>
  test_long_row_form           nvec past SHORT and past 8 CU blocks   rows-lds                               fq_kernel<IO, kFmtRows, ., 256>
  test_long_closed_form        nvec past SHORT and past 32 CU blocks  closed-256                             fq_kernel<IO, KIND, ., 256>
  test_f32_row_form            the two short sizes                    rows-lds (fp32 never reads the rows from global memory)
  test_strided_rows            [4, 64, 8, 128] seen as [4, 8, 64, 128]  rows-256 | rows-1024                  fq_rows_kernel

The second short size has full 1024-vector tiles, a ragged tile and a scalar tail on the 1024-thread kernels; the long sizes make every
grid-stride loop start one more pass that is partial.  Every case runs at scale 1 (kDivUnit), 0.037 (kDivFast and its redo) and 2^-110
(outside UniformDiv's band: kDivExact; a bf16 and an fp32 value), observed and not observed, with the amax slot starting at zero, below
the tensor's maximum and above it.  Inputs are the 65 536 bf16 patterns in a fixed permutation, tiled to n (fp32: widened, every other
one with a non-zero low half): once all of them -- a NaN must win the amax -- and once the finite ones alone -- the slot must equal
max(start, max |x|).  The expectation is the oracle's on one period per (format, scale), tiled.  y starts as NaN everywhere with guard
elements on both sides that must still be NaN afterwards."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

LUT_FMT = (0, 0, 0, 0.0, 0.0)                      # QT_FMT_LUT without the row bit: the map as a plain table
LDS_MIN = 1 << 21                                  # csrc kLutLdsMinElems
SHORT_VECS = 256 * 8 * 256 * 2                     # csrc kRowsDirectMaxVecs
GUARD = 8                                          # elements on each side of every output buffer of this module
SCALES = (1.0, 0.037, 2.0 ** -110)                 # kDivUnit | kDivFast (and its redo) | kDivExact
CLOSED = ["e4m3", "int8"]
ROWS = ["posit8_1-rows", "int4-rows"]              # 256 and 512 row words
TABLE = ["posit8_1-table"]


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Io:
    """One tensor dtype of the entry point; tensors travel as their bit patterns (int16 / int32 on the device), so NaN payloads survive."""

    def __init__(self, name, k_per, bits, fn):
        self.name, self.k_per, self.bits, self.fn = name, k_per, bits, fn
        self.bf16 = name == "bf16"
        self.signed = np.int16 if self.bf16 else np.int32
        self.torch = torch.int16 if self.bf16 else torch.int32
        self.esz = 2 if self.bf16 else 4
        self.nan = 0x7FC0 if self.bf16 else 0x7FC00000
        self.inf = 0x7F80 if self.bf16 else 0x7F800000
        self.absmask = 0x7FFF if self.bf16 else 0x7FFFFFFF

    def __repr__(self):
        return self.name

    def magnitude(self, b):
        """What the observer max-accumulates: the fp32 image of |x| as an unsigned integer (a NaN wins, like torch.amax)."""
        return ((b & 0x7FFF).astype(np.uint32) << 16) if self.bf16 else (b & np.uint32(0x7FFFFFFF))

    def canon_dev(self, t):
        """canon_nan16 / canon_nan32 on a device tensor of bit patterns."""
        return torch.where((t & self.absmask) > self.inf, torch.full_like(t, self.nan), t)


BF16 = Io("bf16", 8, np.uint16, "qt_fake_quant_bf16")
F32 = Io("f32", 4, np.uint32, "qt_fake_quant_f32")
IOS = [BF16, F32]


# ---- formats ---------------------------------------------------------------------------------------------------------
_FORMATS = {}


def launch_format(nv, key):
    """(qt_format, device map, the oracle's map) of "<dtype>" (closed form), "<dtype>-table" (plain table) or "<dtype>-rows" (the row
    form as the product launches a table format)."""
    if key not in _FORMATS:
        dtype, _, how = key.partition("-")
        if how == "rows":
            import quantized_training as qt
            from quantized_training.fake_quantize import _launch_format
            lut = qt.get_quantization_map(dtype, torch.device("cuda", torch.cuda.current_device()))
            base = nv.format_for(dtype)
            fmt = _launch_format(base if base.kind == nv.QT_FMT_LUT else nv.QtFormat(*LUT_FMT), lut)
            assert fmt.kind == nv.QT_FMT_LUT and (fmt.p1 & 1), (dtype, "the row form covers this map")
        else:
            fmt = nv.QtFormat(*LUT_FMT) if how == "table" else nv.format_for(dtype)
            assert fmt.kind == {"int8": nv.QT_FMT_INT, "e4m3": nv.QT_FMT_FP_SAT}.get(key, nv.QT_FMT_LUT), key
            assert not (fmt.kind == nv.QT_FMT_LUT and (fmt.p1 & 1))
            lut = torch.from_numpy(nv.build_map_u16(dtype).view(np.int16)).cuda()
        _FORMATS[key] = (fmt, lut, o.get_quantization_map(dtype))
    return _FORMATS[key]


def test_row_form_tables_have_both_sizes(nv):
    assert not (launch_format(nv, ROWS[0])[0].p1 & 2) and (launch_format(nv, ROWS[1])[0].p1 & 2)   # 256 and 512 row words


# ---- sizes and routes ------------------------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def short_sizes(io):
    """The smallest vector launch with a tail, and full 1024-vector tiles + a ragged tile + a scalar tail (16 525 elements in bf16)."""
    return [4096 + 8 + 3, io.k_per * (2 * 1024 + 17) + 5]


def long_size(io, blocks_per_cu):
    """Past SHORT and past one pass of a grid of blocks_per_cu 256-thread workgroups per CU (one vector per lane): the grid-stride loop of
    some workgroups starts one more pass, which is partial; three elements of scalar tail."""
    per_pass = blocks_per_cu * cu_count() * 256
    nvec = max(SHORT_VECS, per_pass) + 3 * 256 + 5
    assert nvec > SHORT_VECS and nvec > per_pass and nvec % per_pass not in (0, per_pass - 1) and (nvec % per_pass) % 256 != 0
    return nvec * io.k_per + 3


def route(nv, io, fmt, n, x_ptr, y_ptr, observed):
    """launch_fq_kind's choice (y given), restated."""
    aligned = x_ptr % 16 == 0 and y_ptr % 16 == 0
    table = fmt.kind == nv.QT_FMT_LUT
    short = n // io.k_per <= SHORT_VECS
    if table and (fmt.p1 & 1) and aligned and n >= 4096:
        if io.bf16 and short:
            return "rows-global-1024" if observed else "rows-global-256"
        return "rows-lds"
    if table and aligned and 4096 <= n < LDS_MIN:
        return "table-global"
    if not aligned or (table and n < LDS_MIN) or n < 4096:
        return "gather"
    if table:
        return "table-lds"
    return "closed-1024" if (observed and short) else "closed-256"


# ---- data, expectations ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def period(io, finite):
    """One period of the input: the bf16 patterns in a fixed permutation (the finite ones alone: 65 280 of them); fp32: widened, every
    other one with a low half of 0x0001, 0x8000 or 0xFFFF (the fold hi16 | (lo16 != 0), fast32's redo).  Shared: do not write to it."""
    p = o.all_bf16_patterns()[np.random.default_rng(20240611).permutation(65536)]
    if finite:
        p = p[(p & 0x7FFF) < 0x7F80]
    if not io.bf16:
        low = np.array([0, 1, 0, 0x8000, 0, 0xFFFF], np.uint32)[np.arange(p.size) % 6]
        p = (p.astype(np.uint32) << 16) | low
        assert np.count_nonzero(p & 0xFFFF) == p.size // 2
    assert finite == bool(np.all(io.magnitude(p) < 0x7F800000))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def period_dev(io, finite):
    return torch.from_numpy(period(io, finite).view(io.signed).copy()).cuda()


@functools.lru_cache(maxsize=None)
def expect_period(io, key, scale, finite):
    """The oracle's fake-quant of one period (canonical bits, on the device); bf16 tensors see the scale rounded to bf16."""
    x, qmap = period(io, finite), o.get_quantization_map(key.partition("-")[0])
    s = np.asarray([scale], np.float32)
    if io.bf16:
        y = o.canon_nan16(o.fq_bf16(x, qmap, o.f32_to_bf16(s)))
    else:
        y = o.canon_nan32(o.fq_f32(x.view(np.float32), qmap, s).view(np.uint32))
    return torch.from_numpy(y.view(io.signed).copy()).cuda()


def tiled(base, n):
    """A fresh device tensor: `base` repeated to n elements."""
    return base.repeat(-(-n // base.numel()))[:n].clone()


def max_magnitude(io, finite, n):
    p = period(io, finite)
    return int(io.magnitude(p[:min(n, p.size)]).max())


def slot_starts(maxmag):
    """Slot contents before an observed launch: zero, a value below the tensor's maximum, a value above it."""
    return [0, maxmag >> 1, min(maxmag + 0x00800000, 0x7FFFFFFF)]


# ---- launches --------------------------------------------------------------------------------------------------------
def check_y(io, ybuf, lo, exp, what):
    n = exp.numel()
    assert bool((ybuf[:lo] == io.nan).all()) and bool((ybuf[lo + n:] == io.nan).all()), ("wrote outside y",) + what
    got = io.canon_dev(ybuf[lo:lo + n])
    if not torch.equal(got, exp):
        bad = torch.nonzero(got != exp).reshape(-1)[:8].cpu().tolist()
        raise AssertionError(what + ("first mismatches at", bad))


def check_amax(ad, start, maxmag, finite, what):
    slot = int(ad.cpu().numpy().view(np.uint32)[0])
    assert slot == max(start, maxmag), what + (hex(slot), hex(start), hex(maxmag))
    assert (maxmag < 0x7F800000) if finite else (maxmag > 0x7F800000 and slot > 0x7F800000), what   # finite maxima | a NaN pattern won


def check_route(nv, io, key, n, want, x_off=0, y_off=0):
    """qt_fake_quant_bf16 / _f32 on n elements: every scale x {all patterns, finite ones} x {not observed, observed from three slot
    contents}, output and slot against the oracle.  want = {observed: route}; x_off / y_off: elements into a 16-byte aligned allocation."""
    fmt, lut, _ = launch_format(nv, key)
    fn = getattr(nv.lib(), io.fn)
    nan = int(np.array([io.nan], io.bits).view(io.signed)[0])
    ybuf = torch.empty(n + 2 * GUARD + y_off, dtype=io.torch, device="cuda")
    lo = GUARD + y_off
    yd = ybuf[lo:lo + n]
    for finite in (False, True):
        xbuf = torch.zeros(n + x_off, dtype=io.torch, device="cuda")
        xd = xbuf[x_off:]
        xd.copy_(tiled(period_dev(io, finite), n))
        assert xd.data_ptr() % 16 == (x_off * io.esz) % 16 and yd.data_ptr() % 16 == (lo * io.esz) % 16
        maxmag = max_magnitude(io, finite, n)
        for scale in SCALES:
            exp = tiled(expect_period(io, key, scale, finite), n)
            sd = torch.tensor([scale], dtype=torch.float32, device="cuda")
            for start in [None] + slot_starts(maxmag):
                what = (io, key, n, scale, "finite" if finite else "all", start)
                observed = start is not None
                got = route(nv, io, fmt, n, xd.data_ptr(), yd.data_ptr(), observed)
                assert got == want[observed], (got, want) + what
                ad = torch.from_numpy(np.array([start], np.uint32).view(np.int32)).cuda() if observed else None
                ybuf.fill_(nan)
                nv.check(fn(xd.data_ptr(), yd.data_ptr(), n, ctypes.byref(fmt), lut.data_ptr(), sd.data_ptr(),
                            ad.data_ptr() if observed else None, stream()), io.fn)
                torch.cuda.synchronize()
                check_y(io, ybuf, lo, exp, what)
                if observed:
                    check_amax(ad, start, maxmag, finite, what)


def both(name):
    return {False: name, True: name}


# ---- 1. the element gather ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CLOSED + ROWS + TABLE)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_element_gather(nv, io, key):
    """fq_gather_kernel: fewer than 4096 elements, and 9000 elements with x and y an odd number of elements into their allocations."""
    check_route(nv, io, key, 4095, both("gather"))
    check_route(nv, io, key, 9000, both("gather"), x_off=1, y_off=1)


# ---- 2. short vector routes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CLOSED)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_short_closed_form(nv, io, key):
    for n in short_sizes(io):
        check_route(nv, io, key, n, {False: "closed-256", True: "closed-1024"})


@pytest.mark.parametrize("key", ROWS)
def test_short_row_form(nv, key):
    """bf16: the row words read where they lie, in global memory behind the map; observed on 1024 threads."""
    for n in short_sizes(BF16):
        check_route(nv, BF16, key, n, {False: "rows-global-256", True: "rows-global-1024"})


@pytest.mark.parametrize("key", ROWS)
def test_f32_row_form(nv, key):
    """fp32 tensors never read the row words from global memory: the LDS-rows kernel at every size."""
    for n in short_sizes(F32):
        check_route(nv, F32, key, n, both("rows-lds"))


@pytest.mark.parametrize("key", TABLE)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_short_plain_table(nv, io, key):
    """The plain table gathered from global memory by 16-byte vectors (n < 2^21)."""
    for n in short_sizes(io):
        check_route(nv, io, key, n, both("table-global"))


# ---- 3. the plain table in LDS -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", TABLE)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_plain_table_in_lds(nv, io, key):
    """n >= 2^21: 1024-thread workgroups that stage the 128 KiB map, tiles of 4096 vectors, a ragged tile and a scalar tail."""
    n = LDS_MIN + 8 * 1024 * 5 + 3
    assert n // io.k_per <= SHORT_VECS
    check_route(nv, io, key, n, both("table-lds"))


# ---- 4. long routes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ROWS)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_long_row_form(nv, io, key):
    """Row words in LDS, eight 256-thread workgroups per CU."""
    check_route(nv, io, key, long_size(io, 8), both("rows-lds"))


@pytest.mark.parametrize("key", CLOSED)
@pytest.mark.parametrize("io", IOS, ids=repr)
def test_long_closed_form(nv, io, key):
    """Past SHORT an observed pass runs 256-thread workgroups too, 32 of them per CU."""
    check_route(nv, io, key, long_size(io, 32), both("closed-256"))


# ---- 5. strided rows -> contiguous -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["e4m3", "posit8_1-rows"])
def test_strided_rows(nv, key):
    """qt_fake_quant_rows_bf16 on a [4, 64, 8, 128] storage seen as [4, 8, 64, 128] (a projection's [B, S, H, D] as [B, H, S, D]): the
    contiguous result is the oracle's, transposed; an observed pass of this size runs 1024-thread workgroups."""
    io = BF16
    fmt, lut, _ = launch_format(nv, key)
    B, S, H, D = 4, 64, 8, 128
    n = B * S * H * D
    nvec = n // 8
    nan = int(np.array([io.nan], io.bits).view(io.signed)[0])
    ybuf = torch.empty(n + 2 * GUARD, dtype=io.torch, device="cuda")
    yd = ybuf[GUARD:GUARD + n]
    for finite in (False, True):
        xd = tiled(period_dev(io, finite), n)
        assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
        maxmag = max_magnitude(io, finite, n)
        for scale in SCALES:
            exp = tiled(expect_period(io, key, scale, finite), n).view(B, S, H, D).transpose(1, 2).contiguous().view(-1)
            sd = torch.tensor([scale], dtype=torch.float32, device="cuda")
            for start in [None] + slot_starts(maxmag):
                what = (key, scale, "finite" if finite else "all", start)
                observed = start is not None
                got = "rows-1024" if (observed and nvec <= SHORT_VECS) else "rows-256"         # qt_fake_quant_rows_bf16's choice, restated
                assert got == ("rows-1024" if observed else "rows-256"), what
                ad = torch.from_numpy(np.array([start], np.uint32).view(np.int32)).cuda() if observed else None
                ybuf.fill_(nan)
                nv.check(nv.lib().qt_fake_quant_rows_bf16(xd.data_ptr(), yd.data_ptr(), B, H, S, D, S * H * D, D, H * D, ctypes.byref(fmt),
                                                          lut.data_ptr(), sd.data_ptr(), ad.data_ptr() if observed else None, stream()), "rows")
                torch.cuda.synchronize()
                check_y(io, ybuf, GUARD, exp, what)
                if observed:
                    check_amax(ad, start, maxmag, finite, what)
