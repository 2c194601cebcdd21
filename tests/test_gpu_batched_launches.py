"""The many-tensors-per-launch kernels of csrc/qt_elementwise.hip, item by item at ragged sizes:

  qt_fake_quant_multi_bf16       every per-tensor weight fake-quantizer of a step (fake_quantize.BatchedWeightFakeQuant)
  qt_fake_quant_multi_bf16_fp8   the FP8-codes-only weight passes of an evaluation forward (fused.BatchedWeightCodes)
  qt_fake_quant_bf16_fp8_multi   up to four sibling weights back to back into one buffer
  qt_scale_update(_multi)        the delayed-scaling update of one / of every observing fake-quantizer

Every comparison is bit for bit (NaNs canonicalised): against the CPU oracle, and against the single launch the item replaces.  Every
tensor a launch may touch is carved out of ONE allocation filled with a sentinel byte, every output with a guard band on both sides;
after the launch every byte that is not an output still holds what it held -- inputs, guards, the slots of unobserved items."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

pytestmark = pytest.mark.gpu

QT_OK, QT_ERR_BAD_ARG, QT_ERR_UNALIGNED = 0, -2, -3


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def host_u16(t):
    return t.cpu().numpy().view(np.uint16)


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits_of(t):
    """The bit patterns of a bf16 / fp32 tensor, NaNs canonicalised."""
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return o.canon_nan16(host_u16(t.view(torch.int16))).reshape(-1)
    return o.canon_nan32(host_u32(t.view(torch.int32))).reshape(-1)


# ---- one allocation, guarded outputs ---------------------------------------------------------------------------------
SENTINEL = 0xA5
GUARD = 128               # bytes on each side of an output: 64 bf16 elements, 128 FP8 codes, 32 fp32 words


class Arena:
    """Plans a byte image on the host (`put` an input, reserve an `out`put between two guard bands; every offset 16-byte aligned),
    uploads it as ONE device allocation (`commit`) and, after the launches, checks that every byte outside the outputs is unchanged."""

    def __init__(self):
        self.size = GUARD
        self.parts, self.outs = [], []
        self.dev = None

    def _take(self, nbytes):
        off = (self.size + 15) & ~15
        self.size = off + nbytes
        return off

    def put(self, arr):
        a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        off = self._take(max(a.size, 16))          # (a zero-length tensor keeps a valid, aligned address of its own)
        self.parts.append((off, a.copy()))
        return off

    def out(self, nbytes):
        self._take(GUARD)
        off = self._take(nbytes)
        self._take(GUARD)
        self.mark_out(off, nbytes)
        return off

    def mark_out(self, off, nbytes):
        self.outs.append((off, nbytes))

    def commit(self):
        self.host = np.full(((self.size + 15) & ~15) + GUARD, SENTINEL, np.uint8)
        for off, a in self.parts:
            self.host[off:off + a.size] = a
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        self.base = self.dev.data_ptr()
        assert self.base % 16 == 0
        return self

    def ptr(self, off):
        return self.base + off

    def fetch(self):
        torch.cuda.synchronize()
        self.got = self.dev.cpu().numpy()
        return self

    def read(self, off, count, dtype):
        return self.got[off:off + count * np.dtype(dtype).itemsize].view(dtype).copy()

    def assert_rest_untouched(self, what):
        keep = np.ones(self.host.size, bool)
        for off, nbytes in self.outs:
            keep[off:off + nbytes] = False
        bad = np.flatnonzero((self.got != self.host) & keep)
        assert bad.size == 0, (what, "bytes outside the outputs changed, first at offsets", bad[:8].tolist())


# ---- the items: sizes, data, scales, observers -----------------------------------------------------------------------
SIZES = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2048, 4097)          # 16-byte vectors (multi_bf16) / 32-byte pairs (multi_bf16_fp8)
SCALES = (1.0, 0.037, 2.0 ** -3, 0.1, 2.0 ** -110, 2.0 ** 105)         # unit | fast: general, power of two, not a bf16 value | exact
COUNTS = (1, 64, 65, 70)                                               # 65, 70: the second round of the 64-lane item scan
BIG_START = 0x7F000000                                                 # an amax slot that already holds a large value
PATTERNS = o.all_bf16_patterns()


def item_size(i):
    return SIZES[i % len(SIZES)]


def item_scale(i):
    return float(np.float32(SCALES[(i + i // len(SIZES)) % len(SCALES)]))


def item_observed(i):
    return (i + i // len(SIZES)) % 2 == 0


def item_start(i):
    return BIG_START if i % 3 == 0 else 0


def permuted_patterns(n, seed, pool=PATTERNS):
    """`n` elements of a seeded permutation of the tiled pattern pool: NaN, +-inf, subnormals, +-0 and saturating values everywhere."""
    reps = max(1, -(-n // pool.size))
    return np.random.default_rng(seed).permutation(np.tile(pool, reps))[:n].astype(np.uint16)


def has_nan(x):
    return bool(np.any((x & 0x7FFF) > 0x7F80))


def amax_bits(x, start=0):
    return max(int(start), int((x & 0x7FFF).max()) << 16) if x.size else int(start)


_DATA, _EXPECT, _SINGLE = {}, {}, {}


def item_data(i):
    if i not in _DATA:
        _DATA[i] = permuted_patterns(8 * item_size(i), 1000 + i)
    return _DATA[i]


def expect_bf16(xbits, dtype, scale):
    """The CPU oracle's fake-quant with the scale rounded to bf16 (scale.to(X.dtype))."""
    qmap = o.get_quantization_map(dtype)
    sb = o.f32_to_bf16(np.array([scale], np.float32))
    return o.canon_nan16(o.fq_bf16(xbits, qmap, sb))


def item_expect(dtype, i):
    if (dtype, i) not in _EXPECT:
        _EXPECT[dtype, i] = expect_bf16(item_data(i), dtype, item_scale(i))
    return _EXPECT[dtype, i]


CLOSED = ("int8", "e4m3", "e5m2")
TABLES = ("posit8_1", "int4")              # maps launched as tables: row form without / with rows of their own for negative inputs


def launch_format(nv, dtype):
    """(format, device map or None) as the product launches `dtype`: closed form (CLOSED), or its map as a table in the row form (TABLES;
    for a dtype that has a closed form this is the call without a format descriptor, FusedAmaxObsFakeQuantFunction's qt_format = None)."""
    if dtype in CLOSED:
        return nv.format_for(dtype), None
    import quantized_training as qt
    from quantized_training.fake_quantize import _launch_format
    lut = qt.get_quantization_map(dtype, torch.device("cuda", torch.cuda.current_device()))
    base = nv.format_for(dtype)
    fmt = _launch_format(base if base.kind == nv.QT_FMT_LUT else nv.QtFormat(nv.QT_FMT_LUT, 0, 0, 0.0, 0.0), lut)
    assert fmt.kind == nv.QT_FMT_LUT and (fmt.p1 & 1), (dtype, "the row form covers this map")
    return fmt, lut


def single_fq(nv, dtype, xbits, scale, start):
    """One qt_fake_quant_bf16 launch (start = None: not observed) -> (canonical output bits, amax slot afterwards)."""
    fmt, lut = launch_format(nv, dtype)
    x = torch.from_numpy(xbits.view(np.int16)).cuda()
    y = torch.empty_like(x)
    sc = torch.tensor([scale], dtype=torch.float32, device="cuda")
    am = torch.from_numpy(np.array([start or 0], np.uint32).view(np.int32)).cuda()
    nv.check(nv.lib().qt_fake_quant_bf16(x.data_ptr(), y.data_ptr(), x.numel(), ctypes.byref(fmt), lut.data_ptr() if lut is not None else None,
                                         sc.data_ptr(), am.data_ptr() if start is not None else None, stream()), "qt_fake_quant_bf16")
    torch.cuda.synchronize()
    return o.canon_nan16(host_u16(y)), int(host_u32(am)[0])


def item_single(nv, dtype, i):
    if (dtype, i) not in _SINGLE:
        _SINGLE[dtype, i] = single_fq(nv, dtype, item_data(i), item_scale(i), item_start(i) if item_observed(i) else None)
    return _SINGLE[dtype, i]


def test_table_formats_cover_both_row_table_sizes(nv):
    """The table formats of this module load 256 and 512 row words (csrc fq_multi_kernel: `fmt.p1 & 2`)."""
    seen = {bool(launch_format(nv, dt)[0].p1 & 2) for dt in TABLES}
    assert seen == {False, True}, seen


class FqLaunch:
    """The arena and item array of one qt_fake_quant_multi_bf16 launch over `specs`: (bits, scale, observed, start) per item."""

    def __init__(self, specs):
        self.specs = specs
        ar = self.arena = Arena()
        self.x = [ar.put(x) for x, _, _, _ in specs]
        self.scale = ar.put(np.array([s for _, s, _, _ in specs], np.float32))
        self.slots = ar.put(np.array([st for _, _, _, st in specs], np.uint32))
        for i, (_, _, obs, _) in enumerate(specs):
            if obs:
                ar.mark_out(self.slots + 4 * i, 4)           # (the slots of unobserved items stay among the bytes that must not change)
        self.y = [ar.out(2 * x.size) for x, _, _, _ in specs]
        ar.commit()
        rows, tiles = [], 0
        for i, (x, _, obs, _) in enumerate(specs):
            nvec = x.size // 8
            rows.append([ar.ptr(self.x[i]), ar.ptr(self.y[i]), ar.ptr(self.scale + 4 * i), ar.ptr(self.slots + 4 * i) if obs else 0, nvec, tiles])
            tiles += (nvec + 1023) // 1024
        self.tiles = tiles
        self.items = torch.tensor(rows, dtype=torch.int64, device="cuda")          # [count, 6], as BatchedWeightFakeQuant builds it

    def run(self, nv, dtype):
        fmt, lut = launch_format(nv, dtype)
        nv.check(nv.lib().qt_fake_quant_multi_bf16(self.items.data_ptr(), len(self.specs), self.tiles, ctypes.byref(fmt),
                                                   lut.data_ptr() if lut is not None else None, stream()), "qt_fake_quant_multi_bf16")
        self.arena.fetch()                                                          # (synchronizes; items / lut are alive until here)
        return self

    def output(self, i):
        return o.canon_nan16(self.arena.read(self.y[i], self.specs[i][0].size, np.uint16))

    def slot(self, i):
        return int(self.arena.read(self.slots + 4 * i, 1, np.uint32)[0])


# ---- 1. qt_fake_quant_multi_bf16 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("dtype", CLOSED + TABLES)
def test_multi_bf16_items_equal_the_oracle_and_their_single_launches(nv, dtype, count):
    """Item i of one launch == the oracle's fake-quant of tensor i at its own (bf16-rounded) scale == its own qt_fake_quant_bf16 launch,
    amax slot included; one launch mixes the unit, fast and exact division branches, observed and unobserved items, empty and
    pre-filled slots, and sizes on both sides of the 1024-vector tile."""
    assert sum(8 * item_size(i) for i in range(count)) < 1_000_000
    assert count < 6 or {item_scale(i) for i in range(count)} == {float(np.float32(s)) for s in SCALES}
    specs = [(item_data(i), item_scale(i), item_observed(i), item_start(i)) for i in range(count)]
    run = FqLaunch(specs).run(nv, dtype)
    for i, (x, scale, obs, start) in enumerate(specs):
        got = run.output(i)
        assert np.array_equal(got, item_expect(dtype, i)), (dtype, count, i, "oracle", x.size, scale)
        single_y, single_slot = item_single(nv, dtype, i)
        assert np.array_equal(got, single_y), (dtype, count, i, "single launch", x.size, scale)
        if obs:
            assert run.slot(i) == single_slot, (dtype, count, i, hex(run.slot(i)), hex(single_slot))
            if not has_nan(x):
                assert run.slot(i) == amax_bits(x, start), (dtype, count, i, hex(run.slot(i)))
            assert run.slot(i) >= start                                            # max-accumulated, never overwritten
    run.arena.assert_rest_untouched((dtype, count))


def test_multi_bf16_zero_length_item_between_two(nv):
    """An item of no vectors owns no tile (its first_tile is its successor's): both neighbours are computed, its own slot stays."""
    a, b = permuted_patterns(8 * 257, 7), permuted_patterns(8 * 1025, 8)
    empty = np.zeros(0, np.uint16)
    for dtype in ("e4m3", TABLES[1]):
        for specs in ([(a, 0.037, True, 0), (empty, 0.5, True, 0x1234), (b, 1.0, True, 0)],
                      [(empty, 0.5, True, 0x1234), (a, 0.1, False, 0), (b, 2.0 ** -110, True, BIG_START), (empty, 2.0, True, 0x1234)]):
            run = FqLaunch(specs).run(nv, dtype)
            for i, (x, scale, obs, start) in enumerate(specs):
                if x.size == 0:
                    assert run.slot(i) == start
                    continue
                assert np.array_equal(run.output(i), expect_bf16(x, dtype, scale)), (dtype, i)
                want_y, want_slot = single_fq(nv, dtype, x, scale, start if obs else None)
                assert np.array_equal(run.output(i), want_y), (dtype, i)
                if obs:
                    assert run.slot(i) == want_slot, (dtype, i)
            run.arena.assert_rest_untouched(dtype)


def test_multi_bf16_contract_edges(nv):
    L = nv.lib()
    x = permuted_patterns(8 * 257, 3)
    run = FqLaunch([(x, 0.5, True, 0), (x, 1.0, False, 0)])
    fmt = nv.format_for("e4m3")
    call = lambda items, count, tiles, f, lut=None: L.qt_fake_quant_multi_bf16(items, count, tiles, ctypes.byref(f), lut, stream())  # noqa: E731
    items = run.items.data_ptr()
    # nothing to do: QT_OK, and nothing is written
    assert call(items, 0, run.tiles, fmt) == QT_OK
    assert call(items, 2, 0, fmt) == QT_OK
    # formats the launch does not take: a table format without the row form, the identity format
    plain = torch.from_numpy(nv.build_map_u16("posit8_1").view(np.int16)).cuda()
    assert call(items, 2, run.tiles, nv.QtFormat(nv.QT_FMT_LUT, 0, 0, 0.0, 0.0), plain.data_ptr()) == QT_ERR_BAD_ARG
    assert call(items, 2, run.tiles, nv.QtFormat(nv.QT_FMT_IDENTITY, 0, 0, 0.0, 0.0)) == QT_ERR_BAD_ARG
    # an item array that is not 8-byte aligned
    assert call(items + 4, 1, 1, fmt) == QT_ERR_UNALIGNED
    run.arena.fetch()
    run.arena.outs = []
    run.arena.assert_rest_untouched("declined launches")
    del plain


# ---- 2. qt_fake_quant_multi_bf16_fp8 ---------------------------------------------------------------------------------
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
FINITE_SMALL = PATTERNS[(PATTERNS & 0x7FFF) < 0x43E0]          # |x| < 448: below the maximum of both formats
NON_FINITE = PATTERNS[(PATTERNS & 0x7FFF) >= 0x7F80]           # +-inf and every NaN


_DATA8, _CODES = {}, {}


def item_data8(i):
    """Tensor i of the FP8 launches (16 * SIZES elements).  Every 20th pair of items is special: one holds only finite values below
    the format's maximum (every tile takes the hardware conversion), one only NaN / inf (every vector takes the closed form)."""
    if i not in _DATA8:
        n = 16 * item_size(i)
        pool = {8: FINITE_SMALL, 7: NON_FINITE}.get(i % 20, PATTERNS)
        _DATA8[i] = permuted_patterns(n, 2000 + i, pool)
    return _DATA8[i]


def decode_fp8(codes, dtype):
    """FP8 codes -> canonical bf16 bits of their values (OCP, torch's float8 types), as test_fp8_side_output compares them."""
    t = torch.from_numpy(codes.copy()).view(FP8[dtype]).float().bfloat16().view(torch.int16)
    return o.canon_nan16(t.numpy().view(np.uint16))


def expect_code_values(xbits, dtype):
    """The oracle's quantized values at unit scale."""
    return o.canon_nan16(o.quantize_bf16(xbits, o.get_quantization_map(dtype), o.f32_to_bf16(np.array([1.0], np.float32))))


def single_codes(nv, dtype, xbits, key=None):
    """qt_fake_quant_bf16_fp8 with y = NULL at unit scale: the codes of one tensor."""
    if key is not None and (dtype, key) in _CODES:
        return _CODES[dtype, key]
    fmt = nv.format_for(dtype)
    x = torch.from_numpy(xbits.view(np.int16)).cuda()
    y8 = torch.full((max(x.numel(), 16),), SENTINEL, dtype=torch.uint8, device="cuda")
    one = torch.ones(1, dtype=torch.float32, device="cuda")
    nv.check(nv.lib().qt_fake_quant_bf16_fp8(x.data_ptr(), None, y8.data_ptr(), x.numel(), ctypes.byref(fmt), one.data_ptr(), None, stream()),
             "qt_fake_quant_bf16_fp8")
    torch.cuda.synchronize()
    codes = y8.cpu().numpy()[:x.numel()]
    if key is not None:
        _CODES[dtype, key] = codes
    return codes


def test_fp8_items_hold_both_special_kinds():
    for pool, i in ((FINITE_SMALL, 8), (NON_FINITE, 7)):
        assert pool.size > 0 and np.isin(item_data8(i), pool).all() and i < min(c for c in COUNTS if c > 1)
        assert item_size(i) > 1024                              # more than one tile of that kind
    assert not has_nan(FINITE_SMALL) and np.all((NON_FINITE & 0x7F80) == 0x7F80)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("dtype", sorted(FP8))
def test_multi_bf16_fp8_items_equal_the_oracle_and_their_single_launches(nv, dtype, count):
    ar = Arena()
    xs = [ar.put(item_data8(i)) for i in range(count)]
    ys = [ar.out(item_data8(i).size) for i in range(count)]
    ar.commit()
    rows, tiles = [], 0
    for i in range(count):
        npair = item_size(i)
        rows.append([ar.ptr(xs[i]), ar.ptr(ys[i]), npair, tiles])
        tiles += (npair + 1023) // 1024
    items = torch.tensor(rows, dtype=torch.int64, device="cuda")
    fmt = nv.format_for(dtype)
    nv.check(nv.lib().qt_fake_quant_multi_bf16_fp8(items.data_ptr(), count, tiles, ctypes.byref(fmt), stream()), "qt_fake_quant_multi_bf16_fp8")
    ar.fetch()
    for i in range(count):
        x = item_data8(i)
        got = ar.read(ys[i], x.size, np.uint8)
        assert np.array_equal(got, single_codes(nv, dtype, x, key=i)), (dtype, count, i, "single launch")
        assert np.array_equal(decode_fp8(got, dtype), expect_code_values(x, dtype)), (dtype, count, i, "oracle")
    ar.assert_rest_untouched((dtype, count))
    # a format that has no FP8 codes is declined; so is nothing to do accepted without a launch
    bad = nv.format_for("int8")
    assert nv.lib().qt_fake_quant_multi_bf16_fp8(items.data_ptr(), count, tiles, ctypes.byref(bad), stream()) == QT_ERR_BAD_ARG
    assert nv.lib().qt_fake_quant_multi_bf16_fp8(items.data_ptr(), 0, tiles, ctypes.byref(fmt), stream()) == QT_OK
    assert nv.lib().qt_fake_quant_multi_bf16_fp8(items.data_ptr(), count, 0, ctypes.byref(fmt), stream()) == QT_OK
    before = ar.got
    assert np.array_equal(ar.fetch().got, before)


# ---- 3. qt_fake_quant_bf16_fp8_multi ---------------------------------------------------------------------------------
NS_LISTS = ([16], [0], [16, 0, 48], [0, 272, 16], [272, 16, 0], [16, 4096 * 16 + 16], [4096 * 16 + 16, 16, 0, 272], [0, 0, 16, 0])


def _fp8_multi_arena(ns, seed):
    ar = Arena()
    data = [permuted_patterns(n, seed + j) for j, n in enumerate(ns)]
    xs = [ar.put(x) for x in data]
    y8 = ar.out(sum(ns)) if sum(ns) else ar.put(np.full(16, SENTINEL, np.uint8))
    return ar.commit(), data, xs, y8


@pytest.mark.parametrize("ns", NS_LISTS, ids=lambda ns: "-".join(map(str, ns)))
@pytest.mark.parametrize("dtype", sorted(FP8))
def test_fp8_multi_is_the_concatenation_of_the_single_launches(nv, dtype, ns):
    """Counts 1 to 4 with a zero-length tensor at the front, in the middle and at the end: tensor i's codes start at ns[0] + ... + ns[i-1]."""
    ar, data, xs, y8 = _fp8_multi_arena(ns, 3000)
    fmt = nv.format_for(dtype)
    px = (ctypes.c_void_p * len(ns))(*[ar.ptr(x) for x in xs])
    pn = (ctypes.c_size_t * len(ns))(*ns)
    nv.check(nv.lib().qt_fake_quant_bf16_fp8_multi(px, pn, len(ns), ar.ptr(y8), ctypes.byref(fmt), stream()), "qt_fake_quant_bf16_fp8_multi")
    ar.fetch()
    got = ar.read(y8, sum(ns), np.uint8)
    want = np.concatenate([single_codes(nv, dtype, x) if x.size else np.zeros(0, np.uint8) for x in data])
    assert np.array_equal(got, want), (dtype, ns)
    assert np.array_equal(decode_fp8(got, dtype), expect_code_values(np.concatenate(data), dtype)), (dtype, ns)
    ar.assert_rest_untouched((dtype, ns))


def test_fp8_multi_declines(nv):
    L = nv.lib()
    ar, data, xs, y8 = _fp8_multi_arena([32, 48, 16, 64, 16], 3100)
    fmt = nv.format_for("e4m3")

    def call(ptrs, ns, count, y):
        px = (ctypes.c_void_p * len(ptrs))(*ptrs)
        pn = (ctypes.c_size_t * len(ns))(*ns)
        return L.qt_fake_quant_bf16_fp8_multi(px, pn, count, y, ctypes.byref(fmt), stream())

    ptrs, ns, y = [ar.ptr(x) for x in xs], [32, 48, 16, 64, 16], ar.ptr(y8)
    assert call(ptrs, ns, 0, y) == QT_ERR_BAD_ARG
    assert call(ptrs, ns, 5, y) == QT_ERR_BAD_ARG
    assert call(ptrs, [32, 40, 16, 64, 16], 3, y) == QT_ERR_UNALIGNED          # ns[1] is no multiple of 16
    assert call([ptrs[0], ptrs[1] + 2] + ptrs[2:], ns, 3, y) == QT_ERR_UNALIGNED
    assert call(ptrs, ns, 3, y + 8) == QT_ERR_UNALIGNED
    assert call([ptrs[0], None] + ptrs[2:], ns, 3, y) == QT_ERR_BAD_ARG
    bad = nv.format_for("int8")
    px, pn = (ctypes.c_void_p * 5)(*ptrs), (ctypes.c_size_t * 5)(*ns)
    assert L.qt_fake_quant_bf16_fp8_multi(px, pn, 3, y, ctypes.byref(bad), stream()) == QT_ERR_BAD_ARG
    ar.fetch()
    ar.outs = []
    ar.assert_rest_untouched("declined launches")


# ---- 4. qt_scale_update / qt_scale_update_multi ----------------------------------------------------------------------
def scale_update_ref(hist, scale, quant_max, pow2):
    """include/qt_hip.h (fake_quantize.py:230-242) in numpy fp32: amax = max over the history, NaN propagating; the history rolled by
    one, slot 0 zeroed; scale = amax / quant_max, the old scale kept when amax <= 0 or non-finite; optionally 2^ceil(log2 scale), the
    logarithm rounded to fp32.  Returns (history, scale) afterwards."""
    L = hist.shape[0]
    with np.errstate(all="ignore"):
        amax = np.max(hist, axis=0)
        new = np.roll(hist, -1, axis=0) if L > 1 else hist.copy()
        new[0] = 0.0
        sf = (amax / np.float32(quant_max)).astype(np.float32)
        sf = np.where(amax > 0.0, sf, scale)
        sf = np.where(np.isfinite(amax), sf, scale).astype(np.float32)
        if pow2:
            lg = np.log2(sf.astype(np.float64)).astype(np.float32)
            sf = np.exp2(np.ceil(lg).astype(np.float64)).astype(np.float32)
    return new, sf


KINDS = ("random", "zero", "negative", "nan", "inf", "subnormal", "tiny")


def make_state(L, C, seed, first_kind):
    """A [L, C] history and C old scales; channel c is of kind KINDS[(c + first_kind) % 7]."""
    rng = np.random.default_rng(seed)
    h = (rng.random((L, C)) * 10.0 ** rng.uniform(-3, 3, (L, C))).astype(np.float32) + np.float32(1e-6)
    for c in range(C):
        kind = KINDS[(c + first_kind) % len(KINDS)]
        if kind == "zero":
            h[:, c] = 0.0
        elif kind == "negative":
            h[:, c] = -h[:, c]
        elif kind == "nan":
            h[rng.integers(L), c] = np.nan
        elif kind == "inf":
            h[rng.integers(L), c] = np.inf
        elif kind == "subnormal":
            h[:, c] = rng.integers(1, 0x00800000, L).astype(np.uint32).view(np.float32)
        elif kind == "tiny":                                   # normal values whose quotient by quant_max is subnormal
            h[:, c] = rng.integers(0x00800000, 0x01000000, L).astype(np.uint32).view(np.float32)
    scale = rng.uniform(0.55, 1.9, C).astype(np.float32)        # (no power of two: a kept scale shows, with and without force_pow2)
    return h, scale


class StateImage:
    """Histories and scales of several fake-quantizers carved out of one arena; `expected()` is the image the update must leave."""

    def __init__(self, states):
        ar = self.arena = Arena()
        self.states, self.where = states, []
        for hist, scale, _, _ in states:
            self.where.append((ar.out(hist.nbytes), ar.out(scale.nbytes)))
        ar.commit()
        for (hist, scale, _, _), (ho, so) in zip(states, self.where):
            ar.host[ho:ho + hist.nbytes] = hist.reshape(-1).view(np.uint8)
            ar.host[so:so + scale.nbytes] = scale.view(np.uint8)
        ar.dev.copy_(torch.from_numpy(ar.host.copy()))

    def single_launches(self, nv):
        for (hist, scale, qmax, pow2), (ho, so) in zip(self.states, self.where):
            nv.check(nv.lib().qt_scale_update(self.arena.ptr(ho), hist.shape[0], hist.shape[1], self.arena.ptr(so), float(qmax), int(pow2),
                                              stream()), "qt_scale_update")
        return self.arena.fetch().got.copy()

    def multi_launch(self, nv):
        ar = self.arena
        i64, i32 = dict(dtype=torch.int64, device="cuda"), dict(dtype=torch.int32, device="cuda")
        arrays = [torch.tensor([ar.ptr(ho) for ho, _ in self.where], **i64),
                  torch.tensor([s[0].shape[0] for s in self.states], **i32), torch.tensor([s[0].shape[1] for s in self.states], **i32),
                  torch.tensor([ar.ptr(so) for _, so in self.where], **i64),
                  torch.tensor([float(s[2]) for s in self.states], dtype=torch.float32, device="cuda"),
                  torch.tensor([int(s[3]) for s in self.states], **i32)]
        nv.check(nv.lib().qt_scale_update_multi(*[a.data_ptr() for a in arrays], len(self.states), stream()), "qt_scale_update_multi")
        return ar.fetch().got.copy(), arrays

    def expected(self):
        img = self.arena.host.copy()
        for (hist, scale, qmax, pow2), (ho, so) in zip(self.states, self.where):
            new, sf = scale_update_ref(hist, scale, qmax, pow2)
            img[ho:ho + hist.nbytes] = new.reshape(-1).view(np.uint8)
            img[so:so + scale.nbytes] = sf.view(np.uint8)
        return img

    def assert_image(self, got, want, what):
        """Whole arena: guards byte for byte, histories and scales bit for bit with NaNs canonicalised."""
        g, w = o.canon_nan32(got.view(np.uint32)), o.canon_nan32(want.view(np.uint32))
        for k, ((hist, scale, qmax, pow2), (ho, so)) in enumerate(zip(self.states, self.where)):
            L, C = hist.shape
            gs, ws = g[so // 4:so // 4 + C], w[so // 4:so // 4 + C]
            bad = np.flatnonzero(gs != ws)
            assert bad.size == 0, (what, k, "scale", (L, C, qmax, pow2), "channels", bad[:6].tolist(), [hex(v) for v in gs[bad[:6]]],
                                   [hex(v) for v in ws[bad[:6]]])
            assert np.array_equal(g[ho // 4:ho // 4 + L * C], w[ho // 4:ho // 4 + L * C]), (what, k, "history", (L, C, qmax, pow2))
        assert np.array_equal(g, w), (what, "bytes outside the histories and scales changed")


LS, CS, QMAXES = (1, 2, 5, 16), (1, 3, 128, 129, 300), (448.0, 127.0, 1.0)


_STATES = []


def _all_states():
    """(history, old scales, quant_max, force_pow2) of every case, built once and only read.  The kind of channel 0 advances from one
    state to the next of the same (C, force_pow2): its 12 states put every kind into every channel count, C = 1 included."""
    if not _STATES:
        nth = {}
        for L in LS:
            for C in CS:
                for qmax in QMAXES:
                    for pow2 in (0, 1):
                        k = nth[C, pow2] = nth.get((C, pow2), -1) + 1
                        _STATES.append(make_state(L, C, seed=len(_STATES), first_kind=k) + (qmax, pow2))
    return _STATES


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("L", LS)
def test_scale_update_equals_the_restatement(nv, L, C):
    """Scale AND whole history after one qt_scale_update, for every quant_max and both force_pow2 values; the channels hold random
    positives, all-zero, all-negative, NaN, +inf, subnormal histories and histories whose scale is subnormal."""
    states = [s for s in _all_states() if s[0].shape == (L, C)]
    assert len(states) == 6
    img = StateImage(states)
    img.assert_image(img.single_launches(nv), img.expected(), "qt_scale_update")


def test_scale_update_multi_equals_the_single_launches(nv):
    """One qt_scale_update_multi over 37 fake-quantizers of every (L, C, quant_max, force_pow2) kind == their own launches == the
    restatement; nothing to do is QT_OK, a missing array is declined."""
    states = _all_states()[::3][:37]
    assert len(states) == 37 and {s[0].shape[1] for s in states} == set(CS) and {s[0].shape[0] for s in states} == set(LS)
    one, many = StateImage(states), StateImage(states)
    want = one.expected()
    got_single = one.single_launches(nv)
    got_multi, arrays = many.multi_launch(nv)
    many.assert_image(got_multi, want, "qt_scale_update_multi")
    one.assert_image(got_single, want, "qt_scale_update")
    assert np.array_equal(o.canon_nan32(got_multi.view(np.uint32)), o.canon_nan32(got_single.view(np.uint32)))
    L = nv.lib()
    ptrs = [a.data_ptr() for a in arrays]
    assert L.qt_scale_update_multi(*ptrs, 0, stream()) == QT_OK
    assert L.qt_scale_update_multi(None, None, None, None, None, None, 0, stream()) == QT_OK
    for k in range(len(ptrs)):
        assert L.qt_scale_update_multi(*[None if j == k else p for j, p in enumerate(ptrs)], len(states), stream()) == QT_ERR_BAD_ARG
    assert np.array_equal(many.arena.fetch().got, got_multi)                        # (none of those wrote)


def test_scale_update_power_of_two_boundary(nv):
    """force_pow2 next to every power of two: 2^k for k in -60..60, each offset by -6..+6 fp32 ulps (1573 channels, L = 1, quant_max = 1)
    against torch.pow(2, torch.ceil(torch.log2(sf))) on a CPU fp32 tensor -- the device the golden fixtures come from."""
    base = np.array([np.float32(2.0) ** k for k in range(-60, 61)], np.float32).view(np.uint32).astype(np.int64)
    vals = (base[:, None] + np.arange(-6, 7)[None, :]).reshape(-1).astype(np.uint32).view(np.float32)
    assert vals.size == 1573 and np.all(np.isfinite(vals)) and np.all(vals > 0)
    hist = vals.reshape(1, -1).copy()
    img = StateImage([(hist, np.full(vals.size, 3.0, np.float32), 1.0, 1)])
    got = img.single_launches(nv)
    sf = torch.from_numpy(vals.copy())
    want = torch.pow(2, torch.ceil(torch.log2(sf))).numpy()
    assert want.dtype == np.float32
    ho, so = img.where[0]
    got_scale = got[so:so + 4 * vals.size].view(np.float32)
    bad = np.flatnonzero(got_scale.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, ("2^ceil(log2 sf)", [(float(vals[i]).hex(), float(got_scale[i]), float(want[i])) for i in bad[:8]])
    img.assert_image(got, img.expected(), "qt_scale_update")                        # the restatement agrees; history zeroed, guards intact


# ---- 5. the Python builders, without a model -------------------------------------------------------------------------
def test_builders_equal_the_ordinary_calls(nv):
    """BatchedScaleUpdate + BatchedWeightFakeQuant on bare (fake-quantizer, weight) pairs against twins called the ordinary way: outputs,
    scales and amax histories bit for bit over three rounds; pairs the batch must leave out; a weight changed between launch and call."""
    import quantized_training as qt
    from quantized_training import fake_quantize as fqm
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator().manual_seed(11)

    def weight(shape, dtype=torch.bfloat16, transposed=False):
        w = (torch.randn(shape[::-1] if transposed else shape, generator=gen) * 0.05).to(dtype).to(dev)
        return w.t() if transposed else w

    def make_fq(spec):
        """`dtype[,qs=..][,qmax=..][,ahl=..][,ax=..]` -> module; an observing one gets the format's maximum and 16 slots by default."""
        dtype, *rest = spec.split(",")
        f = dict(item.split("=") for item in rest)
        kw = {}
        if "qs" in f:
            kw = dict(qscheme=f["qs"], quant_max=float(f.get("qmax", {"e4m3": 448.0, "int8": 127.0}.get(dtype))),
                      amax_history_len=int(f.get("ahl", 16)))
            if "ax" in f:
                kw["ch_axis"] = int(f["ax"])
        return qt.FusedAmaxObsFakeQuantize(dtype=dtype, device=dev, **kw)

    def pair_and_twin(spec, shape, **kw):
        w = weight(shape, **kw)
        out = []
        for _ in range(2):
            fq = make_fq(spec)
            out.append((fq, torch.nn.Parameter(w.clone() if w.is_contiguous() else w.t().clone().t())))
        return out

    batched = [pair_and_twin(*a) for a in (
        ("e4m3,qs=per_tensor_symmetric,ahl=4", (1, 8)), ("e4m3,qs=per_tensor_symmetric,ahl=4", (129, 72)), ("e4m3", (3, 8)),
        ("int8,qs=per_tensor_symmetric,ahl=3", (3, 8)), ("int8,qs=per_tensor_symmetric,ahl=1", (1025, 8)),
        ("int8,qs=per_tensor_symmetric", (1024, 8)), ("posit8_1,qs=per_tensor_symmetric,qmax=64,ahl=2", (1024, 8)),
        ("posit8_1", (1025, 8)), ("posit8_1,qs=per_tensor_symmetric,qmax=64", (129, 72)))]
    changed = pair_and_twin("e4m3,qs=per_tensor_symmetric,ahl=2", (1025, 8))          # its weight changes between launch and call
    left_out = [pair_and_twin("int8,qs=per_tensor_symmetric,ahl=3", (3, 7)),           # numel % 8 != 0
                pair_and_twin("e4m3,qs=per_tensor_symmetric,ahl=4", (16, 8), transposed=True),
                pair_and_twin("int8,qs=per_tensor_symmetric,ahl=2", (3, 8), dtype=torch.float32),
                pair_and_twin("int8,qs=per_channel_symmetric,ax=0,ahl=2", (16, 8))]
    assert not left_out[1][0][1].is_contiguous() and not left_out[1][1][1].is_contiguous()
    everyone = batched + [changed] + left_out
    mine, twins = [p[0] for p in everyone], [p[1] for p in everyone]

    def same_state(what):
        for k, ((fq, W), (tfq, TW)) in enumerate(zip(mine, twins)):
            assert np.array_equal(bits_of(W), bits_of(TW)), (what, k, "weight")
            assert np.array_equal(bits_of(fq.scale), bits_of(tfq.scale)), (what, k, "scale", fq.scale, tfq.scale)
            assert fq.amax_history.shape == tfq.amax_history.shape
            assert np.array_equal(bits_of(fq.amax_history), bits_of(tfq.amax_history)), (what, k, "history", fq.amax_history, tfq.amax_history)

    for (fq, W), (tfq, TW) in zip(mine, twins):                                       # warm-up: the histories exist
        assert np.array_equal(bits_of(fq(W)), bits_of(tfq(TW)))
    same_state("warm-up")

    from quantized_training import precomputed as pre
    upd = fqm.BatchedScaleUpdate([fq for fq, _ in mine], dev)
    wq = fqm.BatchedWeightFakeQuant(mine, dev)
    try:
        launched = {id(fq): y for g in wq.groups for (fq, _), y in zip(g.members, g.outs)}  # where the launch leaves each member's result
        members = set(launched)
        assert members == {id(p[0][0]) for p in batched + [changed]}, "exactly the eligible pairs are batched"
        assert len(wq) == len(batched) + 1 and len(wq.groups) >= 3
        assert any(g.fmt.kind == nv.QT_FMT_LUT and (g.fmt.p1 & 1) for g in wq.groups)
        observing = [fq for fq, _ in mine if fq._observe]
        assert {id(f) for f in upd.fqs} == {id(f) for f in observing} and len(observing) >= 10

        for rnd in range(3):
            with torch.no_grad():
                for (fq, W), (tfq, TW) in zip(mine, twins):
                    bump = (torch.randn(W.shape, generator=gen) * 0.02 * (rnd + 1)).to(W.dtype).to(dev)
                    W.add_(bump)
                    TW.add_(bump)
            upd.launch()
            assert all(pre.take_preupdate(f.amax_history) for f in observing)          # every one is marked (taking a mark removes it:
            for f in observing:                                                        # put it back)
                pre.mark_preupdated(f.amax_history)
            wq.launch()
            assert all(pre.PRE.peek(fq) is not None for fq, _ in mine if id(fq) in members)
            precomputed = bits_of(pre.PRE.peek(changed[0][0]).payload)
            with torch.no_grad():
                changed[0][1].mul_(2)                                                  # amax only grows: the observer state stays comparable
                changed[1][1].mul_(2)
            for k, ((fq, W), (tfq, TW)) in enumerate(zip(mine, twins)):
                y, want = fq(W), tfq(TW)
                assert y.shape == want.shape and y.dtype == want.dtype
                assert np.array_equal(bits_of(y), bits_of(want)), (rnd, k)
                if fq is changed[0][0]:
                    assert not np.array_equal(bits_of(y), precomputed), "the call returned fq(W as it was at the launch)"
                    assert y.data_ptr() != launched[id(fq)].data_ptr()
                elif id(fq) in members:
                    assert y.data_ptr() == launched[id(fq)].data_ptr(), "the call found the launch's result"
            torch.cuda.synchronize()
            same_state(rnd)
            for fq, _ in mine:
                assert pre.PRE.peek(fq) is None
                assert fq.amax_history.numel() == 0 or not pre.take_preupdate(fq.amax_history)
    finally:
        upd.forget()
        wq.forget()
