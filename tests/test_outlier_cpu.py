"""The outlier side path, the parts that need no GPU: what qt_filter_outlier_* / qt_spmm_csr_* answer to every call they decline -- before
their first HIP call, so host addresses stand in for device memory --, every reason for which the routers of
quantized_training/outlier.py hand a call back to the composite (on CPU stand-ins: the device test is lifted and the library replaced
by a recorder; every other predicate is the real one), and that the operators on CPU tensors still give the reference's results."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from quantized_training import _native, mx_gemm, outlier
from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_UNALIGNED

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_BUF = ctypes.create_string_buffer(4096 + 64)
P = (ctypes.addressof(_BUF) + 63) & ~63              # stands in for every device pointer
ODD = P + 1                                          # off every element size
c_int, c_long, c_float, c_void_p = ctypes.c_int, ctypes.c_long, ctypes.c_float, ctypes.c_void_p


def test_symbols_are_exported_with_their_signatures():
    L = _native.lib()
    assert L.qt_abi_version() == 3 and _native.ABI_VERSION == 3
    flt = (c_int, [c_void_p] * 5 + [c_long, c_long, c_float, c_long, c_void_p])
    spmm = (c_int, [c_void_p] * 3 + [c_long, c_long, c_void_p, c_long, c_long, c_int, c_void_p, c_long, c_long, c_int, c_int, c_void_p, c_int,
                                     c_void_p, c_void_p])
    for name, want in (("qt_filter_outlier_bf16", flt), ("qt_filter_outlier_f32", flt), ("qt_spmm_csr_bf16", spmm), ("qt_spmm_csr_f32", spmm)):
        assert hasattr(L, name) and _native.SIGNATURES[name] == want, name
    header = open(os.path.join(os.path.dirname(G), "..", "include", "qt_hip.h")).read()
    for name in ("qt_filter_outlier_bf16", "qt_filter_outlier_f32", "qt_spmm_csr_bf16", "qt_spmm_csr_f32"):
        assert f"int {name}(" in header
    assert "decomposed.py:450-507" in header and "decomposed.py:510-566" in header


# ---- the entry points' declines ----------------------------------------------------------------------------------------------------------
def _filter(f32=False, **kw):
    a = dict(x=P, inlier=P, data=P, indices=P, indptr=P, rows=4, cols=8, threshold=1.0, max_nnz=1)
    a.update(kw)
    fn = _native.lib().qt_filter_outlier_f32 if f32 else _native.lib().qt_filter_outlier_bf16
    return fn(a["x"], a["inlier"], a["data"], a["indices"], a["indptr"], a["rows"], a["cols"], a["threshold"], a["max_nnz"], None)


FILTER_DECLINES = [(f"NULL {p}", {p: None}, QT_ERR_BAD_ARG) for p in ("x", "inlier", "data", "indices", "indptr")]
FILTER_DECLINES += [
    ("rows 0", dict(rows=0), QT_ERR_BAD_ARG), ("cols 0", dict(cols=0), QT_ERR_BAD_ARG), ("rows -1", dict(rows=-1), QT_ERR_BAD_ARG),
    ("rows 2^31 - 1", dict(rows=2 ** 31 - 1, cols=1), QT_ERR_BAD_ARG), ("cols 2^31 - 1", dict(rows=1, cols=2 ** 31 - 1), QT_ERR_BAD_ARG),
    ("rows cols = 2^31", dict(rows=2 ** 16, cols=2 ** 15), QT_ERR_BAD_ARG),
    ("max_nnz -1", dict(max_nnz=-1), QT_ERR_BAD_ARG), ("max_nnz above the element count", dict(max_nnz=33), QT_ERR_BAD_ARG),
]
FILTER_DECLINES += [(f"{p} off its element size", {p: ODD}, QT_ERR_UNALIGNED) for p in ("x", "inlier", "data", "indices", "indptr")]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in FILTER_DECLINES])
def test_filter_outlier_declines_before_the_first_hip_call(kw, code, f32):
    assert _filter(f32, **kw) == code


def _spmm(f32=False, **kw):
    a = dict(data=P, indices=P, indptr=P, cap=8, rows=4, b=P, N=16, K=64, kn=0, scale=P, srows=16, scols=2, div0=1, div1=32, code=None, ncode=0, y=P)
    a.update(kw)
    fn = _native.lib().qt_spmm_csr_f32 if f32 else _native.lib().qt_spmm_csr_bf16
    return fn(a["data"], a["indices"], a["indptr"], a["cap"], a["rows"], a["b"], a["N"], a["K"], a["kn"], a["scale"], a["srows"], a["scols"],
              a["div0"], a["div1"], a["code"], a["ncode"], a["y"], None)


SPMM_DECLINES = [(f"NULL {p}", {p: None}, QT_ERR_BAD_ARG) for p in ("data", "indices", "indptr", "b", "y")]
SPMM_DECLINES += [
    ("rows -1", dict(rows=-1), QT_ERR_BAD_ARG), ("N -1", dict(N=-1), QT_ERR_BAD_ARG), ("K 0", dict(K=0), QT_ERR_BAD_ARG),
    ("capacity -1", dict(cap=-1), QT_ERR_BAD_ARG), ("rows 2^31 - 1", dict(rows=2 ** 31 - 1), QT_ERR_BAD_ARG),
    ("N 2^31 - 1", dict(N=2 ** 31 - 1, srows=2 ** 31 - 1), QT_ERR_BAD_ARG), ("capacity 2^31 - 1", dict(cap=2 ** 31 - 1), QT_ERR_BAD_ARG),
    ("scale rows short of N", dict(srows=15), QT_ERR_BAD_ARG), ("scale columns short of K / 32", dict(scols=1), QT_ERR_BAD_ARG),
    ("scale divisor 0", dict(div1=0), QT_ERR_BAD_ARG), ("[K, N] with the [N, K] scale", dict(kn=1), QT_ERR_BAD_ARG),
    ("a codebook of 257", dict(code=P, ncode=257), QT_ERR_BAD_ARG), ("a codebook of 0", dict(code=P, ncode=0), QT_ERR_BAD_ARG),
    ("K beyond one operand row in LDS", dict(K=90000, scols=2813), QT_ERR_BAD_ARG),
]
SPMM_DECLINES += [(f"{p} off its element size", {p: ODD}, QT_ERR_UNALIGNED) for p in ("data", "indices", "indptr", "b", "scale", "y")]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in SPMM_DECLINES])
def test_spmm_csr_declines_before_the_first_hip_call(kw, code, f32):
    assert _spmm(f32, **kw) == code


@pytest.mark.parametrize("kw", [pytest.param(dict(rows=0), id="no rows"), pytest.param(dict(N=0, srows=1), id="no features")])
def test_spmm_csr_without_output_is_ok_without_a_launch(kw):
    assert _spmm(**kw) == 0


# ---- the routers -------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records the calls the routers make, lets `hook` (if set) act as the kernel, and answers `rc`."""

    def __init__(self, rc=0):
        self.rc, self.calls, self.hook = rc, [], None

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name,) + args)
            if self.hook is not None:
                self.hook(name, args)
            return self.rc
        return call


@pytest.fixture
def lifted(monkeypatch):
    """The routers with their device test lifted (CPU tensors count as device tensors) and the library replaced by a recorder."""
    rec = _Recorder()
    monkeypatch.setattr(outlier, "_on_device", lambda t: isinstance(t, torch.Tensor))
    monkeypatch.setattr(outlier, "_capturing", lambda: True)          # (the eager read of indptr[-1] would see unwritten memory)
    monkeypatch.setattr(outlier, "_stream_ptr", lambda t: None)
    monkeypatch.setattr(outlier._native, "lib", lambda: rec)
    monkeypatch.setenv("QT_MX_GEMM", "1")
    outlier.STATS.reset()
    mx_gemm.STATS.reset()
    return rec


def _csr_problem(dtype=torch.bfloat16, N=24, K=64, transposed=False):
    data = torch.ones(6, dtype=dtype)
    idx = torch.tensor([1, 5, 9, 0, 63, 7], dtype=torch.int32)
    ptr = torch.tensor([0, 2, 2, 6], dtype=torch.int32)
    B = torch.ones((K, N) if transposed else (N, K), dtype=dtype)
    scale = torch.ones((K // 32, N) if transposed else (N, K // 32), dtype=dtype)
    return dict(data=data, indices=idx, indptr=ptr, B=B, B_scale=scale, B_code=None, block_size=32, weight_transposed=transposed)


def test_routers_take_the_stand_in_problems(lifted):
    out = outlier.filter_outlier_or_none(torch.zeros(3, 5, 32), 4.09, 0.1)
    assert [tuple(t.shape) for t in out] == [(3, 5, 32), (48,), (48,), (16,)] and out[2].dtype == out[3].dtype == torch.int32
    name, *args = lifted.calls[0]
    assert name == "qt_filter_outlier_f32" and args[5:9] == [15, 32, float(np.float32(4.09)), 48]
    out = outlier.filter_outlier_or_none(torch.zeros(4, 8, dtype=torch.bfloat16), 4.09, 0.0)
    name, *args = lifted.calls[1]
    assert name == "qt_filter_outlier_bf16" and args[2] is None and args[3] is None and args[5:9] == [4, 8, 4.09375, 0]
    y = outlier.spmm_csr_or_none(**_csr_problem())
    name, *args = lifted.calls[2]
    assert y.shape == (3, 24) and y.dtype == torch.bfloat16 and name == "qt_spmm_csr_bf16"
    assert args[3:5] == [6, 3] and args[6:9] == [24, 64, 0] and args[10:14] == [24, 2, 1, 32] and args[14] is None and args[15] == 0
    y = outlier.spmm_csr_or_none(**_csr_problem(torch.float32, transposed=True))
    name, *args = lifted.calls[3]
    assert y.shape == (3, 24) and name == "qt_spmm_csr_f32" and args[6:9] == [24, 64, 1] and args[10:14] == [2, 24, 32, 1]
    p = _csr_problem()
    p.update(B_scale=None, block_size=None, B_code=torch.arange(16, dtype=torch.bfloat16))
    assert outlier.spmm_csr_or_none(**p) is not None
    args = lifted.calls[4][1:]
    assert args[9] is None and args[14] is not None and args[15] == 16
    assert (outlier.STATS.native, outlier.STATS.fallback) == (5, 0) and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


def test_scale_is_read_as_expand_reads_it():
    B = torch.zeros(40, 100)
    assert outlier._scale_view(B, torch.zeros(40, 4), 32) == (40, 4, 1, 32)          # a partial last block
    assert outlier._scale_view(B, torch.zeros(2, 100), 32) == (2, 100, 32, 1)
    assert outlier._scale_view(B[:20], torch.zeros(4), 32) == (1, 4, 32, 32)        # one dimension: unsqueezed in front
    assert outlier._scale_view(B, torch.zeros(40, 100), 32) == (40, 100, 1, 1)
    for bad in (torch.zeros(40, 3), torch.zeros(1, 40, 4)):
        assert isinstance(outlier._scale_view(B, bad, 32), str)
    for bs in ((1, 32), None, 0, True):
        assert isinstance(outlier._scale_view(B, torch.zeros(40, 4), bs), str)


FILTER_FALLBACKS = [
    ("fp16", lambda: (torch.zeros(4, 8, dtype=torch.float16), 1.0, 0.05)),
    ("fp64", lambda: (torch.zeros(4, 8, dtype=torch.float64), 1.0, 0.05)),
    ("an empty tensor", lambda: (torch.zeros(0, 8), 1.0, 0.05)),
    ("a scalar", lambda: (torch.zeros(()), 1.0, 0.05)),
    ("an oversize tensor", lambda: (torch.zeros(1, dtype=torch.bfloat16).expand(2 ** 16, 2 ** 15), 1.0, 0.05)),
    ("max_pct above 1", lambda: (torch.zeros(4, 8), 1.0, 1.5)),
    ("a negative max_pct", lambda: (torch.zeros(4, 8), 1.0, -0.5)),
]


@pytest.mark.parametrize("make", [pytest.param(m, id=label) for label, m in FILTER_FALLBACKS])
def test_filter_router_falls_back_and_counts_it(lifted, make):
    assert outlier.filter_outlier_or_none(*make()) is None
    assert lifted.calls == [] and (outlier.STATS.native, outlier.STATS.fallback) == (0, 1)


def _with(**kw):
    return lambda p: p.update(kw)


def _cast(dtype, *keys):
    return lambda p: p.update({k: p[k].to(dtype) for k in keys})


SPMM_FALLBACKS = [
    ("fp16", _cast(torch.float16, "data", "B", "B_scale")),
    ("B of another dtype", _cast(torch.float32, "B")),
    ("a scale of another dtype", _cast(torch.float32, "B_scale")),
    ("a codebook of another dtype", _with(B_code=torch.arange(16.0))),
    ("int64 indices", _cast(torch.int64, "indices")),
    ("int64 indptr", _cast(torch.int64, "indptr")),
    ("a codebook of 65536 entries", _with(B_code=torch.zeros(65536, dtype=torch.bfloat16))),
    ("a codebook of 257 entries", _with(B_code=torch.zeros(257, dtype=torch.bfloat16))),
    ("a two-dimensional codebook", _with(B_code=torch.zeros(4, 4, dtype=torch.bfloat16))),
    ("a tuple block size", _with(block_size=(1, 32))),
    ("no block size with a scale", _with(block_size=None)),
    ("a scale that does not cover B", _with(B_scale=torch.ones(24, 1, dtype=torch.bfloat16))),
    ("a three-dimensional scale", _with(B_scale=torch.ones(1, 24, 2, dtype=torch.bfloat16))),
    ("a three-dimensional B", _with(B=torch.ones(1, 24, 64, dtype=torch.bfloat16))),
    ("two-dimensional data", _with(data=torch.ones(2, 3, dtype=torch.bfloat16))),
    ("fewer indices than data", _with(indices=torch.zeros(5, dtype=torch.int32))),
    ("no rows", _with(indptr=torch.zeros(1, dtype=torch.int32))),
    ("an empty B", _with(B=torch.ones(0, 64, dtype=torch.bfloat16), B_scale=None)),
    ("an oversize B", _with(B=torch.ones(1, dtype=torch.bfloat16).expand(2 ** 31 - 1, 64), B_scale=None)),
    ("an operand that is no tensor of the device", _with(indices=[1, 5, 9, 0, 63, 7])),
]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in SPMM_FALLBACKS])
def test_spmm_router_falls_back_and_counts_it(lifted, change):
    p = _csr_problem()
    change(p)
    assert outlier.spmm_csr_or_none(**p) is None
    assert lifted.calls == [] and (outlier.STATS.native, outlier.STATS.fallback) == (0, 1)


def test_routers_are_governed_by_the_gemm_switch(lifted, monkeypatch):
    monkeypatch.setenv("QT_MX_GEMM", "0")
    assert outlier.filter_outlier_or_none(torch.zeros(4, 8), 1.0, 0.05) is None and outlier.spmm_csr_or_none(**_csr_problem()) is None
    assert lifted.calls == [] and (outlier.STATS.native, outlier.STATS.fallback) == (0, 2)


@pytest.mark.parametrize("rc", [QT_ERR_BAD_ARG, QT_ERR_UNALIGNED])
def test_routers_fall_back_when_the_kernel_declines(lifted, rc):
    lifted.rc = rc
    assert outlier.filter_outlier_or_none(torch.zeros(4, 8), 1.0, 0.05) is None and outlier.spmm_csr_or_none(**_csr_problem()) is None
    assert len(lifted.calls) == 2 and (outlier.STATS.native, outlier.STATS.fallback) == (0, 2)


def test_a_launch_error_is_raised_not_hidden(lifted):
    lifted.rc = 700
    lifted.qt_status_string = lambda code: b"launch failure"
    with pytest.raises(_native.QtError):
        outlier.spmm_csr_or_none(**_csr_problem())


def test_non_contiguous_operands_are_made_contiguous(lifted):
    p = _csr_problem()
    p["B"] = torch.ones(64, 24, dtype=torch.bfloat16).t()
    x = torch.zeros(8, 4).t()
    assert outlier.spmm_csr_or_none(**p) is not None and outlier.filter_outlier_or_none(x, 1.0, 0.5) is not None
    assert lifted.calls[0][7:9] == (24, 64) and lifted.calls[1][6:8] == (4, 8)


def test_eager_reads_are_skipped_while_capturing(lifted, monkeypatch, caplog):
    """Outside a capture the routers read indptr[-1]: filter_outlier warns, spmm_csr raises; inside neither happens."""
    p = _csr_problem()
    p["indptr"] = torch.tensor([0, 2, 2, 9], dtype=torch.int32)
    assert outlier.spmm_csr_or_none(**p) is not None
    monkeypatch.setattr(outlier, "_capturing", lambda: False)
    with pytest.raises(IndexError, match="index 6 is out of bounds for dimension 0 with size 6"):
        outlier.spmm_csr_or_none(**p)
    def seven_entries(name, args):                                  # what the kernels would leave in indptr[rows] (host memory here)
        ctypes.c_int32.from_address(args[4] + 4 * args[5]).value = 7
    lifted.hook = seven_entries
    with caplog.at_level("WARNING", logger="quantized_training.decomposed"):
        outlier.filter_outlier_or_none(torch.zeros(4, 8), 1.0, 0.05)
    assert [r.getMessage() for r in caplog.records] == ["Number of non-zero elements 7 exceeds max_nnz 1, truncating."]


def test_cpu_and_traced_tensors_never_reach_the_library(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(outlier._native, "lib", lambda: rec)
    outlier.STATS.reset()
    ops = torch.ops.quantized_ops
    x = torch.randn(4, 64) * 3
    inl, data, idx, ptr = ops.filter_outlier(x, 4.0, 0.5)
    ops.spmm_csr(data, idx, ptr, torch.ones(8, 64))
    assert outlier.filter_outlier_or_none(x, 4.0, 0.5) is None and outlier.spmm_csr_or_none(data, idx, ptr, torch.ones(8, 64)) is None
    meta = torch.empty(4, 64, device="meta")
    assert not outlier._on_device(meta) and not outlier._on_device(x)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        assert not outlier._on_device(torch.empty(4, 64))
    assert rec.calls == [] and (outlier.STATS.native, outlier.STATS.fallback) == (0, 0)


# ---- the operators on CPU tensors ----------------------------------------------------------------------------------------------------------
def _canon32(t):
    b = t.detach().contiguous().view(torch.int32).numpy().view(np.uint32).copy()
    b[((b & 0x7F800000) == 0x7F800000) & ((b & 0x7FFFFF) != 0)] = 0x7FC00000
    return b


def test_cpu_operators_still_give_the_golden_results():
    arr = np.load(os.path.join(G, "outlier.npz"))
    info = json.load(open(os.path.join(G, "outlier.json")))["op"]
    ops = torch.ops.quantized_ops
    f32 = lambda key, shape: torch.from_numpy(arr[key].view(np.float32).copy()).reshape(shape)
    outlier.STATS.reset()
    x = f32("op__x", (3, 5, 32))
    inl, data, idx, ptr = ops.filter_outlier(x, info["threshold"], info["max_pct"])
    assert np.array_equal(_canon32(inl).reshape(-1), arr["op__inlier"].reshape(-1)) and np.array_equal(_canon32(data), arr["op__data"].reshape(-1))
    assert np.array_equal(idx.numpy().astype(np.int64), arr["op__indices"]) and np.array_equal(ptr.numpy().astype(np.int64), arr["op__indptr"])
    w, ws = f32("op__w", (24, 32)), f32("op__ws", (24, 1))
    assert np.array_equal(_canon32(ops.spmm_csr(data, idx, ptr, w)).reshape(-1), arr["op__y_plain"].reshape(-1))
    assert np.array_equal(_canon32(ops.spmm_csr(data, idx, ptr, w, ws, None, 32)).reshape(-1), arr["op__y_scaled"].reshape(-1))
    assert np.array_equal(_canon32(ops.spmm_csr(data, idx, ptr, w.T.contiguous(), None, None, None, True)).reshape(-1), arr["op__y_transposed"].reshape(-1))
    assert (outlier.STATS.native, outlier.STATS.fallback) == (0, 0)
