"""record_histogram on the device (csrc/qt_histogram.hip, qt_fake_quant_hist_bf16, quantized_training/histogram.py).

Kernel level, through the C ABI: `hist` sits between guard bands (kernel_launch.Guarded); the expected buffer is
fl32(h0 + fl32(bincount of the fp32 exponent fields)) from numpy, and all 254 words and both bands are compared bit for bit; `counts`
and the ticket must read back all-zero after every launch.  Module level: the quantizer with the flag against a CPU twin (which runs the
reference's composite), the route counters, and a captured graph."""
import ctypes
from dataclasses import asdict

import numpy as np
import pytest
import torch

from kernel_launch import GUARD, OK, Guarded, dev, nv, stream, table_format  # noqa: F401

pytestmark = pytest.mark.gpu


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def fields(bits, f16=False):
    """fp32 exponent field of every element's exact fp32 image."""
    if f16:
        return (bits.view(np.float16).astype(np.float32).view(np.uint32) >> 23) & 0xFF
    return (bits.astype(np.uint32) >> 7) & 0xFF


def expected(h0, bits, f16=False):
    c = np.bincount(fields(bits, f16), minlength=256)[1:255]
    return h0.astype(np.float32) + c.astype(np.float32)            # fl32(h0 + fl32(c)): numpy's float32 add rounds once


class Scratch:
    def __init__(self):
        self.words = torch.zeros(257, dtype=torch.int32, device="cuda")

    @property
    def counts(self):
        return self.words.data_ptr()

    @property
    def ticket(self):
        return self.words.data_ptr() + 1024

    def zero(self):
        return not bool(self.words.any())


def hist_buffer(h0):
    g = Guarded((254,), np.float32)
    g.raw[GUARD:GUARD + g.n].copy_(torch.from_numpy(np.ascontiguousarray(h0, np.float32).view(np.uint8).copy()).cuda())
    return g


def run_hist(nv, x, n, h0, sc=None, f16=False, offset=0):
    """x: device int16 tensor; the launch reads n elements from element `offset` on.  Returns hist as uint32 bits."""
    sc = sc or Scratch()
    g = hist_buffer(h0)
    fn = nv.lib().qt_exp_histogram_f16 if f16 else nv.lib().qt_exp_histogram_bf16
    rc = fn(x.data_ptr() + 2 * offset, n, g.ptr, sc.counts, sc.ticket, stream())
    torch.cuda.synchronize()
    assert rc == OK and g.intact() and sc.zero()
    return g.host().view(np.uint32)


def check(nv, bits, h0=None, f16=False, offset=0, sc=None):
    h0 = np.zeros(254, np.float32) if h0 is None else h0
    x = dev(bits)
    got = run_hist(nv, x, bits.size - offset, h0, sc=sc, f16=f16, offset=offset)
    want = expected(h0, bits[offset:], f16).view(np.uint32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    return got


def random_bits(n, seed, scale=1.0):
    from oracle import qt_oracle as o
    rng = np.random.default_rng(seed)
    return o.f32_to_bf16((rng.standard_normal(n) * scale).astype(np.float32))


@pytest.fixture(scope="module")
def plan(nv):
    tile, cap = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert nv.lib().qt_exp_histogram_plan(ctypes.byref(tile), ctypes.byref(cap)) == OK
    assert tile.value == 1024 * 2 * 8 and cap.value % torch.cuda.get_device_properties(0).multi_processor_count == 0
    return tile.value, cap.value


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
def sizes(tile, cap):
    return {"one": 1, "tail_only": 7, "vector_and_tail": 8 + 3, "one_tile": tile, "one_tile_plus_1": tile + 1,
            "ragged_last_tile": 5 * tile + 777,
            "past_grid_clamp": (cap + 3) * tile + 13}          # more tiles than the launcher's largest grid: the grid-stride loop runs twice


@pytest.mark.parametrize("name", ["one", "tail_only", "vector_and_tail", "one_tile", "one_tile_plus_1", "ragged_last_tile", "past_grid_clamp"])
def test_sizes(nv, plan, name):
    n = sizes(*plan)[name]
    h0 = np.linspace(0.0, 253.0, 254, dtype=np.float32)
    check(nv, random_bits(n, seed=n % 1000, scale=8.0), h0)


@pytest.mark.parametrize("offset", [1, 3, 7])
def test_base_pointer_offset_by_elements(nv, plan, offset):
    """A 2-byte aligned base: the scalar head runs up to the first 16-byte boundary."""
    bits = random_bits(plan[0] + 41 + offset, seed=offset, scale=0.01)
    check(nv, bits, offset=offset)
    check(nv, bits[:offset + 3], offset=offset)                   # head longer than the tensor


# ---- data --------------------------------------------------------------------------------------------------------------------------
def test_every_bf16_pattern(nv):
    got = check(nv, np.arange(65536, dtype=np.uint16))
    assert np.all(got.view(np.float32) == 256.0)


def test_every_fp16_pattern(nv):
    got = check(nv, np.arange(65536, dtype=np.uint16), f16=True).view(np.float32)
    assert got[102:112].tolist() == [2.0 * (1 << k) for k in range(10)]       # the subnormals
    assert np.all(got[112:142] == 2048.0) and got[:102].sum() == 0 and got[142:].sum() == 0
    check(nv, np.random.default_rng(1).integers(0, 65536, 70001).astype(np.uint16), f16=True, offset=1)


@pytest.mark.parametrize("what", ["zeros", "nan_inf"])
def test_nothing_counted_leaves_hist_unchanged(nv, what):
    n = 40003
    bits = np.zeros(n, np.uint16)
    if what == "zeros":
        bits[1::2] = 0x8000                                         # -0.0, and fp32-subnormal magnitudes
        bits[2::5] = 0x0041
    else:
        bits[:] = np.array([0x7F80, 0xFF80, 0x7FC0, 0xFFFF, 0x7F81], np.uint16)[np.arange(n) % 5]
    h0 = np.full(254, 3.25, np.float32)
    got = check(nv, bits, h0)
    assert np.array_equal(got, h0.view(np.uint32))


def test_all_equal_million(nv):
    """Every lane on one bin, and a non-zero count that the last workgroup must read back from where the adds were made."""
    got = check(nv, np.full(1 << 20, 0x3F80, np.uint16)).view(np.float32)
    assert got[126] == float(1 << 20) and got.sum() == float(1 << 20)


def test_two_bins_alternating(nv):
    bits = np.where(np.arange(100003) % 2 == 0, 0x3F80, 0xC2C8).astype(np.uint16)
    check(nv, bits)


def test_normal_random(nv):
    check(nv, random_bits(300001, seed=11))


# ---- accumulation ------------------------------------------------------------------------------------------------------------------
def _four_bin_data():
    vals = np.array([0x3F80, 0x4000, 0x4080, 0x3F00], np.uint16)     # bins 126, 127, 128, 125
    reps = [100001, 70003, 33335, 12347]
    return np.concatenate([np.full(r, v, np.uint16) for v, r in zip(vals, reps)])


def test_single_rounding_into_large_entries(nv):
    """h0 of 0.5, 2^24, 2^24 + 2 and 3e7 under odd counts: one rounding of the sum, where a float add per element would stall."""
    h0 = np.zeros(254, np.float32)
    h0[[126, 127, 128, 125]] = [0.5, 2.0 ** 24, 2.0 ** 24 + 2, 3e7]
    got = check(nv, np.random.default_rng(0).permutation(_four_bin_data()), h0).view(np.float32)
    assert got[127] > 2.0 ** 24 and got[128] > 2.0 ** 24 + 2 and got[126] == 100001.5


def test_two_calls_on_one_scratch_and_two_hist_buffers(nv):
    sc = Scratch()
    a, b = random_bits(50001, seed=1), random_bits(20000, seed=2, scale=100.0)
    x_a, x_b = dev(a), dev(b)
    h0 = np.zeros(254, np.float32)
    first = run_hist(nv, x_a, a.size, h0, sc=sc)
    second = run_hist(nv, x_b, b.size, first.view(np.float32), sc=sc)          # the ticket and counts were reset by the first launch
    assert np.array_equal(second, expected(expected(h0, a), b).view(np.uint32))
    other = run_hist(nv, x_b, b.size, np.ones(254, np.float32), sc=sc)          # same scratch, another hist buffer
    assert np.array_equal(other, expected(np.ones(254, np.float32), b).view(np.uint32))
    # back to back without a synchronise in between
    g1, g2 = hist_buffer(h0), hist_buffer(h0)
    L = nv.lib()
    assert L.qt_exp_histogram_bf16(x_a.data_ptr(), a.size, g1.ptr, sc.counts, sc.ticket, stream()) == OK
    assert L.qt_exp_histogram_bf16(x_b.data_ptr(), b.size, g2.ptr, sc.counts, sc.ticket, stream()) == OK
    assert L.qt_exp_histogram_bf16(x_b.data_ptr(), b.size, g1.ptr, sc.counts, sc.ticket, stream()) == OK
    torch.cuda.synchronize()
    assert sc.zero() and g1.intact() and g2.intact()
    assert np.array_equal(g1.host().view(np.uint32), expected(expected(h0, a), b).view(np.uint32))
    assert np.array_equal(g2.host().view(np.uint32), expected(h0, b).view(np.uint32))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(nv):
    sc = Scratch()
    x = dev(random_bits(4096, seed=0))
    g = Guarded((254,), np.float32)
    L = nv.lib()
    for f in (L.qt_exp_histogram_bf16, L.qt_exp_histogram_f16):
        assert f(x.data_ptr(), 4096, None, sc.counts, sc.ticket, stream()) != OK              # null hist
        assert f(x.data_ptr(), 4096, g.ptr, None, sc.ticket, stream()) != OK
        assert f(x.data_ptr(), 4096, g.ptr, sc.counts, None, stream()) != OK
        assert f(None, 4096, g.ptr, sc.counts, sc.ticket, stream()) != OK
        assert f(x.data_ptr(), 1 << 32, g.ptr, sc.counts, sc.ticket, stream()) != OK          # counts are u32 (refused on the host)
        assert f(x.data_ptr() + 1, 4095, g.ptr, sc.counts, sc.ticket, stream()) != OK         # not 2-byte aligned
        assert f(x.data_ptr(), 0, g.ptr, sc.counts, sc.ticket, stream()) == OK                # nothing to do: no launch
    fmt = nv.format_for("e4m3")
    y = torch.empty_like(x)
    assert L.qt_fake_quant_hist_bf16(x.data_ptr(), y.data_ptr(), 4096, ctypes.byref(fmt), None, None, None, None, sc.counts, sc.ticket, stream()) != OK
    assert L.qt_fake_quant_hist_bf16(x.data_ptr(), y.data_ptr(), 1 << 32, ctypes.byref(fmt), None, None, None, g.ptr, sc.counts, sc.ticket, stream()) != OK
    torch.cuda.synchronize()
    assert g.untouched() and sc.zero()


# ---- the fused sibling -------------------------------------------------------------------------------------------------------------
def _format(nv, name):
    if name == "posit8_1":
        fmt, lut = table_format(nv, name)
        assert fmt.p1 & 1                                                            # the row form: the one-launch variant takes it
        return fmt, lut
    return nv.format_for(name), None


FUSED_SIZES = {"one_launch": (3 * 16384 + 8 * 77 + 5, 0), "small": (1000, 0), "unaligned": (20000, 1)}


@pytest.mark.parametrize("where", list(FUSED_SIZES))
@pytest.mark.parametrize("scale", [None, 0.37], ids=["unit", "scaled"])
@pytest.mark.parametrize("observe", [False, True], ids=["plain", "observed"])
@pytest.mark.parametrize("name", ["e4m3", "int8", "posit8_1"])
def test_fused_pass_equals_its_two_parts(nv, name, observe, scale, where):
    """y and the amax slot are qt_fake_quant_bf16's, hist is qt_exp_histogram_bf16's -- in the one-launch variant (16-byte aligned, n >=
    4096, with scalar tail) and where the launcher has no HIST variant (n < 4096; a base off the 16-byte grid: the gather kernel)."""
    n, offset = FUSED_SIZES[where]
    fmt, lut = _format(nv, name)
    bits = random_bits(n + offset, seed=n, scale=5.0)
    x = dev(bits)
    xp = x.data_ptr() + 2 * offset
    s = torch.tensor([scale], dtype=torch.float32, device="cuda") if scale is not None else None
    sp, lp = (s.data_ptr() if s is not None else None), (lut.data_ptr() if lut is not None else None)
    L = nv.lib()
    h0 = np.linspace(1.0, 254.0, 254, dtype=np.float32)

    def amax_slot():
        return torch.zeros(1, dtype=torch.int32, device="cuda")

    y_ref = Guarded((n + offset,), np.uint16)
    a_ref = amax_slot()
    assert L.qt_fake_quant_bf16(xp, y_ref.ptr + 2 * offset, n, ctypes.byref(fmt), lp, sp, a_ref.data_ptr() if observe else None, stream()) == OK
    h_ref = run_hist(nv, x, n, h0, offset=offset)
    assert np.array_equal(h_ref, expected(h0, bits[offset:]).view(np.uint32))

    sc = Scratch()
    y = Guarded((n + offset,), np.uint16)
    a = amax_slot()
    g = hist_buffer(h0)
    assert L.qt_fake_quant_hist_bf16(xp, y.ptr + 2 * offset, n, ctypes.byref(fmt), lp, sp, a.data_ptr() if observe else None, g.ptr, sc.counts,
                                     sc.ticket, stream()) == OK
    torch.cuda.synchronize()
    assert y.intact() and g.intact() and sc.zero()
    assert np.array_equal(y.host()[offset:], y_ref.host()[offset:])
    assert int(a.item()) == int(a_ref.item()) and (int(a.item()) != 0) == observe
    assert np.array_equal(g.host().view(np.uint32), h_ref)


# ---- module level ------------------------------------------------------------------------------------------------------------------
def _module(spec, device, **extra):
    import quantized_training as qt
    kw = asdict(qt.QuantizationSpec.from_str(spec))
    kw.update(extra)
    return qt.FusedAmaxObsFakeQuantize(**kw, record_histogram=True, device=device)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.float().view(torch.int32).numpy()


def _twin_calls(spec, shape, extra, dtype=torch.bfloat16, prepare=None):
    """Three calls on the device module and on its CPU twin (the reference's composite): y, histogram and scale after each."""
    from quantized_training import histogram
    m_gpu, m_cpu = _module(spec, "cuda", **extra), _module(spec, "cpu", **extra)
    histogram.reset_stats()
    g = torch.Generator().manual_seed(17)
    for scale in (1.0, 30.0, 1e-3):
        x = (torch.randn(shape, generator=g) * scale).to(dtype)
        xg = x.cuda()
        if prepare is not None:
            x, xg = prepare(x), prepare(xg)
        with torch.no_grad():
            y_gpu, y_cpu = m_gpu(xg), m_cpu(x)
        assert np.array_equal(_bits(y_gpu), _bits(y_cpu)), (spec, scale, "y")
        assert np.array_equal(_bits(m_gpu.histogram), _bits(m_cpu.histogram)), (spec, scale, "histogram")
        assert np.array_equal(_bits(m_gpu.scale.reshape(-1)), _bits(m_cpu.scale.reshape(-1))), (spec, scale, "scale")
    assert float(m_gpu.histogram.sum()) > 0
    return dict(histogram.STATS)


@pytest.mark.parametrize("shape", [(7, 96), (64, 200)], ids=["two_launch_size", "one_launch_size"])
@pytest.mark.parametrize("spec", ["e4m3", "int8,qs=per_tensor_symmetric", "posit8_1"])
def test_module_fused_route_against_cpu_twin(spec, shape):
    stats = _twin_calls(spec, shape, {})
    assert stats == {"histogram_native": 0, "histogram_fused": 3, "histogram_composite": 3}      # (the CPU twin's three are the composite's)


@pytest.mark.parametrize("spec,extra", [("fp8_e4m3,qs=microscaling,bs=32,ax=-1", {}), ("int8,qs=per_channel_symmetric,ax=0", {}),
                                        ("posit8_1", {"outlier_threshold": 4.0}), ("e4m3", {"outlier_threshold": 1.5})],
                         ids=["microscaling", "per_channel", "outlier_posit", "outlier_e4m3"])
def test_module_standalone_route_against_cpu_twin(spec, extra):
    stats = _twin_calls(spec, (6, 128), extra)
    assert stats == {"histogram_native": 3, "histogram_fused": 0, "histogram_composite": 3}


def test_module_fp16_and_permuted_view_take_the_standalone_launch():
    stats = _twin_calls("e4m3", (6, 128), {}, prepare=lambda t: t.t())                              # dense, not contiguous
    assert stats == {"histogram_native": 3, "histogram_fused": 0, "histogram_composite": 3}
    stats = _twin_calls("e4m3", (6, 128), {}, dtype=torch.float16)
    assert stats == {"histogram_native": 3, "histogram_fused": 0, "histogram_composite": 3}


def test_module_observe_and_quantize_off_still_records():
    from quantized_training import histogram
    m = _module("int8,qs=per_tensor_symmetric", "cuda")
    m.disable_observer()
    m.disable_fake_quant()
    histogram.reset_stats()
    x = torch.randn(33, 65).bfloat16().cuda()
    assert m(x) is x
    assert histogram.STATS == {"histogram_native": 1, "histogram_fused": 0, "histogram_composite": 0}
    assert np.array_equal(m.histogram.cpu().numpy(), expected(np.zeros(254, np.float32), _bits(x).view(np.uint16).reshape(-1)))


def test_module_declines_run_the_composite(monkeypatch):
    stats = _twin_calls("int8,qs=per_tensor_symmetric", (5, 64), {}, dtype=torch.float32)          # fp32 input
    assert stats == {"histogram_native": 0, "histogram_fused": 0, "histogram_composite": 6}
    from quantized_training import histogram
    m = _module("e4m3", "cuda")
    m.histogram = m.histogram.bfloat16()                                                            # what model.to(torch.bfloat16) does
    histogram.reset_stats()
    x = torch.randn(8, 64).bfloat16().cuda()
    m(x)
    assert histogram.STATS == {"histogram_native": 0, "histogram_fused": 0, "histogram_composite": 1} and m.histogram.dtype == torch.bfloat16
    monkeypatch.setenv("QT_HISTOGRAM", "0")
    stats = _twin_calls("e4m3", (64, 200), {})
    assert stats == {"histogram_native": 0, "histogram_fused": 0, "histogram_composite": 6}


def test_captured_module_call_replayed_three_times_equals_three_eager_calls():
    x = (torch.randn(64, 200) * 3).bfloat16().cuda()
    results = {}
    for spec, enabled in (("e4m3", True), ("int8,qs=per_tensor_symmetric", False)):             # the fused and the stand-alone route
        eager, graphed = _module(spec, "cuda"), _module(spec, "cuda")
        if not enabled:                                                                            # quantize and observe off: the histogram launch alone
            for m in (eager, graphed):
                m.disable_observer()
                m.disable_fake_quant()
        with torch.no_grad():
            for _ in range(3):
                y_eager = eager(x)
        graphed._move_to(x.device)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s), torch.no_grad():
            with torch.cuda.graph(g, stream=s):
                y_graph = graphed(x)
        torch.cuda.current_stream().wait_stream(s)
        assert float(graphed.histogram.sum()) == 0.0                                               # capture launches nothing
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(graphed.histogram), _bits(eager.histogram)), spec
        assert np.array_equal(_bits(y_graph), _bits(y_eager)), spec
        assert float(eager.histogram.sum()) == 3.0 * x.numel()
        results[spec] = graphed
