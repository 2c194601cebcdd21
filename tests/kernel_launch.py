"""What the kernel tests that launch through the C ABI share (tests/test_gpu_row_kernels.py, tests/test_gpu_elementwise_ops.py, tests/test_gpu_gemm_fq.py): guarded
output buffers, the two-launch and refused-call checks, the interval check with its per-family statistics, and the single fake-quant
passes the fused variants are compared with.  A plain module, imported by name; it holds no tests."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import qt_oracle as o

GUARD = 128                  # bytes of sentinel in front of and behind every output buffer
SENTINEL = 0xA5
OK = 0


@pytest.fixture(scope="module")
def nv():
    from quantized_training import _native
    assert torch.cuda.is_available(), "these tests need the GPU"
    _native.lib()
    return _native


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(bits):
    """numpy array (uint16 patterns, float32, int32, int64, uint8) -> device tensor of the same bytes."""
    a = np.ascontiguousarray(bits)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


class Guarded:
    """An output buffer between two guard bands."""

    def __init__(self, shape, np_dtype):
        self.shape, self.dtype = tuple(shape), np.dtype(np_dtype)
        self.n = int(np.prod(self.shape)) * self.dtype.itemsize
        self.raw = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def intact(self):
        return bool((self.raw[:GUARD] == SENTINEL).all()) and bool((self.raw[GUARD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.raw == SENTINEL).all())

    def host(self):
        return self.raw[GUARD:GUARD + self.n].cpu().numpy().view(self.dtype).reshape(self.shape)


def launch(fn, specs, what):
    """fn(outs) -> status, twice into fresh guarded buffers: status OK, guards intact, both launches bit-identical.  Returns the host
    arrays of the first launch by name."""
    runs = []
    for _ in range(2):
        outs = {k: Guarded(*v) for k, v in specs.items()}
        assert fn(outs) == OK, what
        torch.cuda.synchronize()
        for k, g in outs.items():
            assert g.intact(), f"{what}: guard band of {k} overwritten"
        runs.append({k: g.host() for k, g in outs.items()})
    for k in specs:
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), f"{what}: {k} differs between two launches"
    return runs[0]


def refused(fn, specs, what):
    outs = {k: Guarded(*v) for k, v in specs.items()}
    assert fn(outs) != OK, what
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert g.untouched(), f"{what}: {k} written by a refused call"


STATS = {}


def inside(iv, got, what, family):
    """got in [lo, hi] everywhere (which is bit equality on the decided elements), NaN where the oracle has NaN."""
    d = iv.distance(got)
    s = STATS.setdefault(family, [1.0, 0])
    s[0], s[1] = min(s[0], iv.decided_share()), max(s[1], int(d.max()))
    if int(d.max()) != 0:
        print(f"[{family}] {what}: {iv.report(got)}")
    assert int(d.max()) == 0, f"{what}: {iv.report(got)}"


def same(a, b, what, where=None):
    a, b = o.canon_nan16(a) if a.dtype == np.uint16 else a, o.canon_nan16(b) if b.dtype == np.uint16 else b
    if where is not None:
        a, b = a[where], b[where]
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} of {a.size} differ"


def print_stats(tag):
    """(with -s) per family: the smallest decided share of a launch's finite elements, ill-conditioned rows included, and the worst
    distance from the interval.  Called from a module's teardown; the statistics start afresh for the next module."""
    for family, (share, worst) in sorted(STATS.items()):
        print(f"\n[{tag}] {family}: smallest decided share {share:.4f}, worst distance from the interval {worst}")
    STATS.clear()


# ---- single passes the fused variants are compared with ---------------------------------------------------------------------------------
def fq8_single(nv, y_bits, dtype):
    """qt_fake_quant_bf16_fp8 at unit scale on y: (bf16 values, FP8 codes)."""
    fmt = nv.format_for(dtype)
    n = y_bits.size
    flat = np.zeros((n + 15) // 16 * 16, np.uint16)               # (that pass takes multiples of 16 elements)
    flat[:n] = y_bits.reshape(-1)
    y = dev(flat)
    out, out8 = torch.empty_like(y), torch.empty(y.numel(), dtype=torch.uint8, device="cuda")
    nv.check(nv.lib().qt_fake_quant_bf16_fp8(y.data_ptr(), out.data_ptr(), out8.data_ptr(), y.numel(), ctypes.byref(fmt), None, None, stream()), "fq8")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)[:n].reshape(y_bits.shape), out8.cpu().numpy()[:n].reshape(y_bits.shape)


def table_format(nv, dtype):
    import quantized_training as qt
    from quantized_training.fake_quantize import _launch_format
    lut = qt.get_quantization_map(dtype, torch.device("cuda"))
    return _launch_format(nv.format_for(dtype), lut), lut


def fq_single(nv, y_bits, fmt, lut):
    y = dev(y_bits)
    out = torch.empty_like(y)
    nv.check(nv.lib().qt_fake_quant_bf16(y.data_ptr(), out.data_ptr(), y.numel(), ctypes.byref(fmt), lut.data_ptr() if lut is not None else None, None, None,
                                         stream()), "fq")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)
