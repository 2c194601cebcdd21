"""The integer block-scaled GEMM (qt_mxi_pack / qt_mxi_gemm), the parts that need no GPU: the two entry points and what they answer to
every call they decline -- before their first HIP call, so aligned host addresses stand in for device memory --, every reason for which
the integer route of mx_gemm hands a problem back (on CPU stand-ins: the device test lifted, the library replaced by a recorder), the
record the producers leave, the codebook check's cache, and that the operators on CPU tensors still are the reference's composite."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from quantized_training import _native, mx_gemm, mx_operand
from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_UNALIGNED
from quantized_training.fake_quantize import get_quantization_map

G = os.path.join(os.path.dirname(__file__), "golden")
_BUF = ctypes.create_string_buffer(4096 + 64)
P = (ctypes.addressof(_BUF) + 63) & ~63              # stands in for every device pointer
BF16, F32 = torch.bfloat16, torch.float32


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_signatures_and_abi_version():
    L = _native.lib()
    assert L.qt_abi_version() == 3 and _native.ABI_VERSION == 3
    for name, nargs in (("qt_mxi_pack", 19), ("qt_mxi_gemm", 15)):
        assert hasattr(L, name) and len(_native.SIGNATURES[name][1]) == nargs and _native.SIGNATURES[name][0] is ctypes.c_int
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "qt_hip.h")).read()
    assert "#define QT_ABI_VERSION 3" in header
    for name in ("qt_mxi_pack", "qt_mxi_gemm"):
        decl = header[header.index(f"int {name}("):]
        assert decl[:decl.index(";")].count(",") + 1 == len(_native.SIGNATURES[name][1])
        assert f"{name} (decomposed.py:304-363" in header


def _gemm(**kw):
    a = dict(a=P, sa=P, b=P, sb=P, bs=64, c=P, f32=0, bias=None, batch=1, M=16, N=16, K=128, ra=0, rb=0)
    a.update(kw)
    return _native.lib().qt_mxi_gemm(a["a"], a["sa"], a["b"], a["sb"], a["bs"], a["c"], a["f32"], a["bias"], a["batch"], a["M"], a["N"], a["K"],
                                     a["ra"], a["rb"], None)


def _pack(**kw):
    a = dict(x=P, s=P, f32=0, code=None, n_code=0, codes=P, scales=P, batch=1, rows=4, K=128, xs=(0, 128, 1), ss=(0, 2, 1), bs=64, bad=None)
    a.update(kw)
    return _native.lib().qt_mxi_pack(a["x"], a["s"], a["f32"], a["code"], a["n_code"], a["codes"], a["scales"], a["batch"], a["rows"], a["K"],
                                     *a["xs"], *a["ss"], a["bs"], a["bad"], None)


GEMM_DECLINES = [(f"NULL {p}", {p: None}, QT_ERR_BAD_ARG) for p in ("a", "sa", "b", "sb", "c")] + [
    ("block size 16", dict(bs=16, K=128), QT_ERR_BAD_ARG), ("block size 48", dict(bs=48, K=96), QT_ERR_BAD_ARG),
    ("block size 256", dict(bs=256, K=256), QT_ERR_BAD_ARG), ("block size 0", dict(bs=0), QT_ERR_BAD_ARG),
    ("K % bs", dict(bs=64, K=96), QT_ERR_BAD_ARG), ("K % bs, 128", dict(bs=128, K=192), QT_ERR_BAD_ARG), ("K 0", dict(K=0), QT_ERR_BAD_ARG),
    ("batch 65536", dict(batch=65536), QT_ERR_BAD_ARG), ("batch -1", dict(batch=-1), QT_ERR_BAD_ARG),
    ("M -1", dict(M=-1), QT_ERR_BAD_ARG), ("N -1", dict(N=-1), QT_ERR_BAD_ARG), ("a batch stride -1", dict(ra=-1), QT_ERR_BAD_ARG),
    ("a off 16 bytes", dict(a=P + 8), QT_ERR_UNALIGNED), ("b off 16 bytes", dict(b=P + 4), QT_ERR_UNALIGNED),
    ("a scales off 4 bytes", dict(sa=P + 2), QT_ERR_UNALIGNED), ("b scales off 4 bytes", dict(sb=P + 1), QT_ERR_UNALIGNED),
    ("bf16 c off 2 bytes", dict(c=P + 1), QT_ERR_UNALIGNED), ("fp32 c off 4 bytes", dict(c=P + 2, f32=1), QT_ERR_UNALIGNED),
    ("fp32 bias off 4 bytes", dict(bias=P + 2, f32=1), QT_ERR_UNALIGNED),
]
PACK_DECLINES = [(f"NULL {p}", {p: None}, QT_ERR_BAD_ARG) for p in ("x", "s", "codes", "scales")] + [
    ("block size 16", dict(bs=16), QT_ERR_BAD_ARG), ("block size 96", dict(bs=96, K=96), QT_ERR_BAD_ARG), ("block size 256", dict(bs=256, K=256), QT_ERR_BAD_ARG),
    ("K % bs", dict(bs=64, K=96), QT_ERR_BAD_ARG), ("batch 65536", dict(batch=65536), QT_ERR_BAD_ARG), ("rows -1", dict(rows=-1), QT_ERR_BAD_ARG),
    ("K -64", dict(K=-64), QT_ERR_BAD_ARG), ("a codebook of 0 entries", dict(code=P, n_code=0), QT_ERR_BAD_ARG),
    ("a codebook of 257 entries", dict(code=P, n_code=257), QT_ERR_BAD_ARG), ("entries without a codebook", dict(n_code=16), QT_ERR_BAD_ARG),
    ("codes off 16 bytes", dict(codes=P + 8), QT_ERR_UNALIGNED), ("scales off 4 bytes", dict(scales=P + 2), QT_ERR_UNALIGNED),
    ("bf16 x off 2 bytes", dict(x=P + 1), QT_ERR_UNALIGNED), ("fp32 x off 4 bytes", dict(x=P + 2, f32=1), QT_ERR_UNALIGNED),
    ("fp32 scale off 4 bytes", dict(s=P + 2, f32=1), QT_ERR_UNALIGNED), ("fp32 codebook off 4 bytes", dict(code=P + 2, n_code=16, f32=1), QT_ERR_UNALIGNED),
    ("flag off 4 bytes", dict(bad=P + 2), QT_ERR_UNALIGNED),
]


@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in GEMM_DECLINES])
def test_gemm_declines_before_the_first_hip_call(kw, code):
    assert _gemm(**kw) == code


@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in PACK_DECLINES])
def test_pack_declines_before_the_first_hip_call(kw, code):
    assert _pack(**kw) == code


def test_empty_problems_are_ok_without_a_launch():
    assert _gemm(M=0) == 0 and _gemm(N=0) == 0 and _gemm(batch=0) == 0
    assert _pack(rows=0) == 0 and _pack(batch=0) == 0 and _pack(K=0) == 0


# ---- the record ------------------------------------------------------------------------------------------------------------------------
def test_float_tables_are_unchanged_and_the_integer_family_has_its_own():
    assert mx_operand.FMT_ID == {"fp8_e4m3": 0, "fp8_e5m2": 1, "fp6_e2m3": 2, "fp6_e3m2": 3, "fp4_e2m1": 4}
    assert mx_operand.BITS == {0: 8, 1: 8, 2: 6, 3: 6, 4: 4}
    assert mx_operand.PAIRS == {(0, 0), (0, 1), (1, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (2, 4), (3, 4)}
    assert mx_operand.NARROW_FIRST == ("fp4_e2m1", "fp6_e2m3", "fp6_e3m2", "fp8_e4m3", "fp8_e5m2")
    assert mx_operand.INT_BITS == {f"int{n}": n for n in range(2, 9)} and not set(mx_operand.INT_BITS) & set(mx_operand.FMT_ID)
    assert mx_operand.INT_BLOCKS == (32, 64, 128) and mx_operand.INT_SLOT != mx_operand.GEMM_SLOT


@pytest.mark.parametrize("pow2", [False, True], ids=["amax", "pow2"])
@pytest.mark.parametrize("fmt,qmax,bs,axis", [("int8", 127.0, 32, -1), ("int6", 31.0, 64, -1), ("int6", 31.0, 64, -2), ("int4", 7.0, 32, -1)])
def test_quantize_and_quantize_mx_leave_the_same_integer_record(fmt, qmax, bs, axis, pow2):
    ops = torch.ops.quantized_ops
    qmap = get_quantization_map(fmt, "cpu")
    x = torch.randn(2, 128, 128, generator=torch.Generator().manual_seed(0)).to(BF16)
    s1, q1 = ops.quantize_mx(x, qmap, [axis], bs, qmax, pow2, None, None)
    s2 = ops.calculate_mx_qparam(x, [axis], bs, qmax, pow2)
    q2 = ops.quantize(x, s2, None, [axis], bs, qmap)
    assert torch.equal(q1, q2) and torch.equal(s1, s2)
    assert mx_operand.format_of(q1) == mx_operand.format_of(q2) == fmt == mx_operand.int_format_of(q1)
    assert mx_operand.is_pow2(s1) == mx_operand.is_pow2(s2) == pow2
    n = mx_operand.INT_BITS[fmt]
    assert bool(((q1 == q1.round()) & (q1 >= -2 ** (n - 1)) & (q1 <= 2 ** (n - 1) - 1)).all())
    q1.add_(1)                                                      # a write in place: the record is stale
    assert mx_operand.int_format_of(q1) is None


def test_no_integer_record_without_an_integer_map_or_with_zero_points():
    ops = torch.ops.quantized_ops
    x = torch.randn(4, 64).to(BF16)
    s = torch.full((4, 2), 0.05, dtype=BF16)
    assert mx_operand.int_format_of(ops.quantize(x, s, None, [-1], 32, get_quantization_map("fp8_e4m3", "cpu"))) is None
    assert mx_operand.int_format_of(ops.quantize(x, s, torch.ones(4, 2, dtype=BF16), [-1], 32, get_quantization_map("int8", "cpu"))) is None
    assert mx_operand.int_format_of(ops.quantize(x, s[:1, :1].reshape(1), None, None, None, get_quantization_map("int8", "cpu"))) is None
    untagged = get_quantization_map("int8", "cpu").clone()         # by tag alone: a map without one is not compared by content
    assert mx_operand.int_format_of_qmap(untagged) is None and mx_operand.int_format_of(ops.quantize(x, s, None, [-1], 32, untagged)) is None
    assert mx_operand.int_format_of_qmap(get_quantization_map("int6", "cpu")) == "int6"
    assert mx_operand.int_format_of_qmap(get_quantization_map("fp8_e4m3", "cpu")) is None


def test_codebook_check_is_cached_by_version():
    code = torch.tensor([-31.0, -16.0, 0.0, 5.0, 31.0], dtype=BF16)
    assert mx_operand.int_codebook_ok(code) and code._qt_mxi_code == (code._version, True)
    code._qt_mxi_code = (code._version, False)                      # the cached answer is the one returned ...
    assert not mx_operand.int_codebook_ok(code)
    code[1] = 0.5                                                   # ... until the codebook is written in place
    assert not mx_operand.int_codebook_ok(code) and code._qt_mxi_code == (code._version, False)
    code[1] = -16.0
    assert mx_operand.int_codebook_ok(code)
    for bad in (torch.tensor([0.0, 128.0]), torch.tensor([-129.0]), torch.tensor([float("nan")]), torch.tensor([float("inf")]),
                torch.zeros(257), torch.zeros(0), torch.zeros(2, 2), torch.arange(4)):
        assert not mx_operand.int_codebook_ok(bad)
    assert mx_operand.int_codebook_ok(torch.arange(-128.0, 128.0))


def test_weight_cache_key_carries_weight_scale_and_codebook_versions():
    w, s, code = torch.zeros(8, 64, dtype=BF16), torch.ones(8, 1, dtype=BF16), torch.arange(16.0).to(BF16)
    calls = []

    def get(c=code, bs=64):
        return mx_operand.int_weight_operand(w, s, c, bs, lambda: calls.append(1) or (len(calls),))
    first = get()
    assert get() is first and len(calls) == 1
    for n, change in enumerate((lambda: w.add_(0), lambda: s.add_(0), lambda: code.add_(0))):
        change()
        assert get() is not first and get() == (n + 2,) and len(calls) == n + 2
    assert get(bs=32) == (5,) and get(c=None) == (6,) and get(c=code.clone()) == (7,)
    assert getattr(w, mx_operand.GEMM_SLOT, None) is None           # the float family's cache is another slot
    refused = mx_operand.int_weight_operand(torch.zeros(2, 64), s, None, 64, lambda: None)
    assert refused is None


# ---- the router ------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records the calls the integer route makes and answers 0."""

    def __init__(self):
        self.calls = []

    def qt_mxi_pack(self, *args):
        self.calls.append(("pack",) + args)
        return 0

    def qt_mxi_gemm(self, *args):
        self.calls.append(("gemm",) + args)
        return 0


@pytest.fixture
def lifted(monkeypatch):
    """The router with its device test lifted and the library replaced, so that CPU tensors reach every later rule of the real predicate."""
    rec = _Recorder()
    monkeypatch.setattr(mx_gemm, "_on_device", lambda t: True)
    monkeypatch.setattr(mx_gemm, "_stream_ptr", lambda t: None)
    monkeypatch.setattr(mx_gemm._native, "lib", lambda: rec)
    monkeypatch.setenv("QT_MX_GEMM", "1")
    mx_gemm.STATS.reset()
    return rec


def _linear(m=6, n=8, k=128, bs=64, dtype=BF16, codes=(False, False)):
    g = torch.Generator().manual_seed(0)
    x, w = torch.randint(-8, 8, (2, m // 2, k), generator=g).to(dtype), torch.randint(-8, 8, (n, k), generator=g).to(dtype)
    p = dict(input=x, weight=w, bias=torch.zeros(n, dtype=dtype), input_scale=torch.ones(2, m // 2, k // bs, dtype=dtype),
             weight_scale=torch.ones(n, k // bs, dtype=dtype), block_size=bs, input_code=None, weight_code=None)
    for which, has in zip(("input", "weight"), codes):
        if has:
            p[which] = p[which].abs()
            p[which + "_code"] = torch.arange(-8.0, 8.0).to(dtype)
        else:
            mx_operand.set_format(p[which], "int6")
    return p


def _matmul(b=2, m=6, n=8, k=128, bs=64, dtype=BF16):
    g = torch.Generator().manual_seed(0)
    a, o = torch.randint(-8, 8, (b, m, k), generator=g).to(dtype), torch.randint(-8, 8, (b, k, n), generator=g).to(dtype)
    mx_operand.set_format(a, "int8"), mx_operand.set_format(o, "int4")
    return dict(a=a, b=o, a_scale=torch.ones(b, m, k // bs, dtype=dtype), b_scale=torch.ones(b, k // bs, n, dtype=dtype), block_size=bs,
                a_code=None, b_code=None)


@pytest.mark.parametrize("codes", [(False, False), (True, False), (False, True), (True, True)], ids=["records", "input code", "weight code", "both codes"])
@pytest.mark.parametrize("bs", [32, 64, 128])
def test_router_takes_the_integer_linear(lifted, bs, codes):
    p = _linear(bs=bs, codes=codes)
    y = mx_gemm.mx_linear_or_none(**p)
    assert y is not None and y.shape == (2, 3, 8) and y.dtype == BF16
    assert [c[0] for c in lifted.calls] == ["pack", "pack", "gemm"]             # the weight (check on), the activation (check off), the GEMM
    wpack, apack, gemm = lifted.calls
    assert wpack[18] is not None and apack[18] is None and (wpack[5], apack[5]) == (16 if codes[1] else 0, 16 if codes[0] else 0)
    assert gemm[5] == bs and gemm[9:15] == (1, 6, 8, 128, 0, 0)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)
    mx_gemm.mx_linear_or_none(**p)                                  # the weight's operand is cached
    assert [c[0] for c in lifted.calls[3:]] == ["pack", "gemm"] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (2, 0)


def test_router_takes_the_integer_matmul(lifted):
    p = _matmul()
    y = mx_gemm.mx_matmul_or_none(**p)
    assert y is not None and y.shape == (2, 6, 8)
    apack, bpack, gemm = lifted.calls
    assert apack[8:17] == (2, 6, 128, 6 * 128, 128, 1, 6 * 2, 2, 1) and bpack[8:17] == (2, 8, 128, 128 * 8, 1, 8, 2 * 8, 1, 8)
    assert gemm[9:15] == (2, 6, 8, 128, 6, 8) and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)
    lifted.calls.clear()
    p["b"] = mx_operand.set_format(p["b"].transpose(-1, -2).contiguous().transpose(-1, -2), "int4")     # K^T: a view of [b, n, k]
    p["b_scale"] = p["b_scale"].transpose(-1, -2).contiguous().transpose(-1, -2)
    assert mx_gemm.mx_matmul_or_none(**p) is not None
    assert lifted.calls[1][8:17] == (2, 8, 128, 8 * 128, 128, 1, 8 * 2, 2, 1)   # packed in place, rows contiguous


def _set(key, value):
    return lambda p: p.update({key: value})


def _forget(key):
    return lambda p: mx_operand.forget(p[key])


def _to(dtype, *keys):
    return lambda p: p.update({k: p[k].to(dtype) for k in keys})


LINEAR_NONE = [
    ("block size 16", _set("block_size", 16)), ("block size 256", _set("block_size", 256)), ("a tuple block size", _set("block_size", (1, 64))),
    ("block size True", _set("block_size", True)), ("fp16", _to(torch.float16, "input", "weight", "input_scale", "weight_scale")),
    ("operands of two dtypes", _to(F32, "weight", "weight_scale")), ("a scale of another dtype", _to(F32, "input_scale")),
    ("no input scale", _set("input_scale", None)), ("no weight scale", _set("weight_scale", None)),
    ("K % block size", lambda p: p.update(_linear(k=96, bs=64))), ("input scale shape", lambda p: p.update(input_scale=p["input_scale"][:, :, :1])),
    ("weight scale shape", lambda p: p.update(weight_scale=p["weight_scale"].t().contiguous())),
    ("weight K", lambda p: p.update(weight=mx_operand.set_format(p["weight"][:, :64].contiguous(), "int6"))),
    ("a 3-d weight", lambda p: p.update(weight=mx_operand.set_format(p["weight"][None], "int6"))),
    ("an empty input", lambda p: p.update(input=mx_operand.set_format(p["input"][:0], "int6"), input_scale=p["input_scale"][:0])),
    ("an input without record or codebook", _forget("input")), ("a weight without record or codebook", _forget("weight")),
    ("a float record on the input", lambda p: mx_operand.set_format(p["input"], "fp8_e4m3")),
    ("a stale record", lambda p: p["input"].add_(0)),
    ("a codebook with a fractional level", _set("weight_code", torch.tensor([0.5, 1.0], dtype=BF16))),
    ("a codebook of 257 entries", _set("weight_code", torch.zeros(257, dtype=BF16))),
    ("a codebook of another dtype", _set("input_code", torch.arange(16.0))),
    ("a bf16 problem above the rule's bound", lambda p: p.update(_linear(m=1024, n=2048, k=512))),
]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in LINEAR_NONE])
def test_linear_router_hands_back_and_counts(lifted, change):
    p = _linear()
    change(p)
    assert mx_gemm.mx_linear_or_none(**p) is None
    assert lifted.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)


def test_a_weight_the_packer_refuses_and_the_switch(lifted, monkeypatch):
    monkeypatch.setattr(mx_gemm, "_int_pack", lambda *a, **k: None if a[-1] else (torch.zeros(1), torch.zeros(1)))
    p = _linear()
    assert mx_gemm.mx_linear_or_none(**p) is None and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)
    assert mx_gemm.mx_linear_or_none(**p) is None and getattr(p["weight"], mx_operand.INT_SLOT)[1] is None        # cached as refused
    monkeypatch.setenv("QT_MX_GEMM", "0")
    mx_gemm.STATS.reset()
    assert mx_gemm.mx_linear_or_none(**_linear()) is None and mx_gemm.mx_matmul_or_none(**_matmul()) is None
    assert lifted.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


MATMUL_NONE = [
    ("block size 16", _set("block_size", 16)), ("fp16", _to(torch.float16, "a", "b", "a_scale", "b_scale")), ("operands of two dtypes", _to(F32, "b", "b_scale")),
    ("batch shapes", lambda p: p.update(b=mx_operand.set_format(p["b"][:1], "int4"), b_scale=p["b_scale"][:1])),
    ("inner extents", lambda p: p.update(b=mx_operand.set_format(p["b"][:, :64].contiguous(), "int4"))),
    ("a scale shape", lambda p: p.update(a_scale=p["a_scale"][:, :, :1])), ("b scale shape", lambda p: p.update(b_scale=p["b_scale"].transpose(-1, -2).contiguous())),
    ("K % block size", lambda p: p.update(_matmul(k=96))), ("a without record", _forget("a")), ("b without record", _forget("b")),
    ("batch above 65535", lambda p: p.update({k: (v.expand((65536,) + tuple(v.shape[1:])) if isinstance(v, torch.Tensor) else v)
                                              for k, v in _matmul(b=1, m=1, n=1, k=64).items()})),
    ("a bf16 problem above the rule's bound", lambda p: p.update(_matmul(b=32, m=512, n=512, k=128))),
]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in MATMUL_NONE])
def test_matmul_router_hands_back_and_counts(lifted, change):
    p = _matmul()
    change(p)
    if p["a"].shape[0] == 65536:                                    # expand() made new tensors: the records go with them
        mx_operand.set_format(p["a"], "int8"), mx_operand.set_format(p["b"], "int4")
    assert mx_gemm.mx_matmul_or_none(**p) is None
    assert lifted.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(mx_gemm._native, "lib", lambda: rec)
    mx_gemm.STATS.reset()
    assert mx_gemm.mx_linear_or_none(**_linear()) is None and mx_gemm.mx_matmul_or_none(**_matmul()) is None and rec.calls == []


@pytest.mark.parametrize("args,takes", [
    ((1024, 4096, 4096, 1, 64, F32), True), ((1024, 11008, 4096, 1, 32, F32), True), ((1024, 1024, 128, 32, 64, F32), True),
    ((16, 128, 64, 1, 32, BF16), True), ((256, 256, 256, 1, 32, BF16), True), ((512, 1024, 1024, 1, 32, BF16), True),
    ((512, 1024, 1056, 1, 32, BF16), False),
    ((1024, 4096, 4096, 1, 64, BF16), False), ((1024, 1024, 128, 32, 64, BF16), False), ((1024, 128, 1024, 32, 64, BF16), False)])
def test_route_rule(args, takes):
    """profiles/mx_int_gemm.txt: fp32 always; bf16 up to 2^29 multiply-adds, the largest measured row that wins."""
    assert mx_gemm._int_route_takes(*args) == takes


# ---- the composite on CPU tensors ----------------------------------------------------------------------------------------------------------
def _restated_linear(x, w, bias, sx, sw, bs, xc, wc):
    """decomposed.py:304-330 restated: codebook lookup, block scales repeated over their blocks, F.linear."""
    dx = (xc[x.to(torch.long)].to(x.dtype) if xc is not None else x) * sx.repeat_interleave(bs, -1)
    dw = (wc[w.to(torch.long)].to(w.dtype) if wc is not None else w) * sw.repeat_interleave(bs, -1)
    return F.linear(dx, dw, bias)


_MX = [c for c in json.load(open(os.path.join(G, "mx.json"))) if c["spec"].startswith(("int", "nf4")) and c["ch_axis"] == -1
       and c["shape"][-1] % c["block_size"] == 0]


@pytest.mark.parametrize("cfg", _MX, ids=[c["name"] for c in _MX])
def test_composite_on_cpu_is_unchanged_for_the_integer_configs(cfg):
    """The int / nf4 configs of tests/golden/mx.json: linear_mx on CPU tensors is the composite restated, bit for bit, and no route is counted."""
    dtype = BF16 if cfg["in"] == "bf16" else F32
    fmt, bs = cfg["spec"].split(",")[0], cfg["block_size"]
    qmap, code = get_quantization_map(fmt, "cpu"), None
    if isinstance(qmap, tuple):
        qmap, code = qmap[0], qmap[1].to(dtype)
    smap = get_quantization_map(cfg["scale_dtype"], "cpu") if cfg["scale_dtype"] else None
    g = torch.Generator().manual_seed(1)
    k = cfg["shape"][-1]
    x, w, bias = torch.randn(6, k, generator=g).to(dtype), torch.randn(10, k, generator=g).to(dtype), torch.randn(10, generator=g).to(dtype)
    sx, xq = torch.ops.quantized_ops.quantize_mx(x, qmap, [-1], bs, cfg["quant_max"], cfg["pow2"], smap, None)
    sw, wq = torch.ops.quantized_ops.quantize_mx(w, qmap, [-1], bs, cfg["quant_max"], cfg["pow2"], smap, None)
    mx_gemm.STATS.reset()
    got = torch.ops.quantized_ops.linear_mx(xq, wq, bias, input_scale=sx, weight_scale=sw, block_size=bs, input_code=code, weight_code=code)
    want = _restated_linear(xq, wq, bias, sx, sw, bs, code, code)
    view = torch.int16 if dtype == BF16 else torch.int32
    assert got.dtype == want.dtype and torch.equal(got.view(view), want.view(view))
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


@pytest.mark.parametrize("name", ["mxfp6_w_int", "nf4_weight"])
def test_converted_integer_graphs_on_cpu_still_match_the_recorded_output(name):
    """The integer configs of tests/golden/pt2e_mx.json: the converted graph on CPU tensors gives the reference's recorded output."""
    import test_pt2e_cpu as t
    from quantized_training import quantize_pt2e as qp
    arr = np.load(os.path.join(G, "pt2e_mx.npz"))
    info, m, xs = t.mx_setup(name, arr)
    gm = qp.prepare_pt2e(m, qp.get_default_quantizer(**info["kw"]), (xs[0],))
    with torch.no_grad():
        gm(xs[0])
        gm(xs[1])
        mx_gemm.STATS.reset()
        y = qp.convert_pt2e(gm)(xs[1])
    assert np.array_equal(t._bits(y), arr[f"{name}__y_converted"]) and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)
