"""conv2d_mx on the block-scaled matrix instruction, the parts that need no GPU: what qt_conv2d_mx answers to every call it declines
-- before its first HIP call, so 16-byte-aligned host addresses stand in for device memory --, every reason for which
mx_conv.mx_conv2d_or_none hands the problem back to the composite (on CPU stand-ins: the device test of the router is lifted and the
library replaced by a recorder), and that the operator on CPU tensors still is the reference's composite bit for bit."""
import ctypes
import itertools
import types

import pytest
import torch

from quantized_training import _native, mx_conv, mx_gemm, mx_operand
from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_BAD_DTYPE, QT_ERR_UNALIGNED

_BUF = ctypes.create_string_buffer(4096 + 64)
P = (ctypes.addressof(_BUF) + 63) & ~63              # stands in for every device pointer
OFF = P + 8                                          # off a 16-byte boundary
POINTERS = ("x", "xs", "w", "ws", "y", "bias")


def _call(**kw):
    a = dict(x=P, xs=P, fx=0, w=P, ws=P, fw=0, y=P, f32=0, bias=P, N=1, H=5, W=5, Cin=64, Cout=16, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1,
             dh=1, dw=1)
    a.update(kw)
    return _native.lib().qt_conv2d_mx(a["x"], a["xs"], a["fx"], a["w"], a["ws"], a["fw"], a["y"], a["f32"], a["bias"], a["N"], a["H"], a["W"],
                                      a["Cin"], a["Cout"], a["kh"], a["kw"], a["sh"], a["sw"], a["ph"], a["pw"], a["dh"], a["dw"], None)


def test_symbol_is_exported_and_declared():
    assert hasattr(_native.lib(), "qt_conv2d_mx") and "qt_conv2d_mx" in _native.SIGNATURES
    assert _native.lib().qt_abi_version() == 3


DECLINES = [(f"NULL {p}", {p: None}, QT_ERR_BAD_ARG) for p in POINTERS if p != "bias"]
DECLINES += [
    ("x format -1", dict(fx=-1), QT_ERR_BAD_ARG), ("x format 5", dict(fx=5), QT_ERR_BAD_ARG),
    ("w format -1", dict(fw=-1), QT_ERR_BAD_ARG), ("w format 5", dict(fw=5), QT_ERR_BAD_ARG),
    ("Cin 0", dict(Cin=0), QT_ERR_BAD_ARG), ("Cin 16", dict(Cin=16), QT_ERR_BAD_ARG), ("Cin 48", dict(Cin=48), QT_ERR_BAD_ARG),
    ("Cin 32, both e2m3", dict(Cin=32, fx=2, fw=2), QT_ERR_UNALIGNED), ("Cin 96, both e3m2", dict(Cin=96, fx=3, fw=3), QT_ERR_UNALIGNED),
    ("Cin 32, e3m2 x and 4-bit w", dict(Cin=32, fx=3, fw=4), QT_ERR_UNALIGNED), ("Cin 96, e2m3 x and 4-bit w", dict(Cin=96, fx=2, fw=4), QT_ERR_UNALIGNED),
    ("kh 0", dict(kh=0), QT_ERR_BAD_ARG), ("kw -1", dict(kw=-1), QT_ERR_BAD_ARG), ("stride 0", dict(sh=0), QT_ERR_BAD_ARG),
    ("stride -1", dict(sw=-1), QT_ERR_BAD_ARG), ("dilation 0", dict(dh=0), QT_ERR_BAD_ARG), ("dilation -2", dict(dw=-2), QT_ERR_BAD_ARG),
    ("padding -1", dict(ph=-1), QT_ERR_BAD_ARG), ("padding -1, columns", dict(pw=-1), QT_ERR_BAD_ARG),
    ("N -1", dict(N=-1), QT_ERR_BAD_ARG), ("H 0", dict(H=0), QT_ERR_BAD_ARG), ("W 0", dict(W=0), QT_ERR_BAD_ARG), ("Cout -1", dict(Cout=-1), QT_ERR_BAD_ARG),
    # extents past 2^31: output pixels, the contraction, the byte sizes of both code arrays
    ("N Ho Wo = 2^31", dict(N=2 ** 11, H=2 ** 10, W=2 ** 10, Cin=32, kh=1, kw=1, ph=0, pw=0), QT_ERR_BAD_ARG),
    ("kh kw Cin = 2^31", dict(H=2 ** 12, W=2 ** 12, Cin=2 ** 11, kh=2 ** 10, kw=2 ** 10, ph=0, pw=0), QT_ERR_BAD_ARG),
    ("x bytes = 2^31", dict(N=1, H=2 ** 13, W=2 ** 12, Cin=64, sh=2 ** 6, sw=2 ** 6, kh=1, kw=1, ph=0, pw=0), QT_ERR_BAD_ARG),
    ("w bytes = 2^31", dict(Cout=2 ** 21, Cin=1024, kh=1, kw=1, ph=0, pw=0), QT_ERR_BAD_ARG),
    ("Cin above 2^24", dict(Cin=2 ** 25), QT_ERR_BAD_ARG),
    ("kh dh = 2^20", dict(H=2 ** 21, W=1, kh=2, kw=1, dh=2 ** 19, ph=0, pw=0), QT_ERR_BAD_ARG),
    ("padding 2^20", dict(pw=2 ** 20), QT_ERR_BAD_ARG),
]
DECLINES += [(f"{p} off 16 bytes", {p: OFF}, QT_ERR_UNALIGNED) for p in POINTERS]
DECLINES += [(f"pair ({a}, {b}) has no kernel", dict(fx=a, fw=b, Cin=64), QT_ERR_BAD_DTYPE)
             for a, b in itertools.product(range(5), repeat=2) if (a, b) not in mx_gemm._PAIRS]


def test_the_pairs_without_a_kernel_are_fifteen():
    assert len(mx_gemm._PAIRS) == 10 and sum(1 for d in DECLINES if d[2] == QT_ERR_BAD_DTYPE) == 15


@pytest.mark.parametrize("kw,code", [pytest.param(kw, code, id=label) for label, kw, code in DECLINES])
def test_declines_before_the_first_hip_call(kw, code):
    assert _call(**kw) == code


@pytest.mark.parametrize("kw", [
    pytest.param(dict(H=2, W=5, kh=3, ph=0), id="Ho = 0"),
    pytest.param(dict(H=5, W=2, kw=5, pw=0), id="Wo < 0"),
    pytest.param(dict(H=3, W=3, dh=3, ph=0), id="dilated filter taller than the plane"),
    pytest.param(dict(N=0), id="N = 0"),
    pytest.param(dict(Cout=0), id="Cout = 0"),
])
def test_empty_output_is_ok_without_a_launch(kw):
    assert _call(**kw) == 0


# ---- the router --------------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the library: records the one call the router may make and answers `rc`."""

    def __init__(self, rc):
        self.rc, self.calls = rc, []

    def qt_conv2d_mx(self, *args):
        self.calls.append(args)
        return self.rc


def _problem(n=2, cin=64, h=6, w=5, cout=8, kh=3, kw=3, bs=32, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-2, 3, (n, cin, h, w), generator=g).to(dtype)
    wt = torch.randint(-2, 3, (cout, cin, kh, kw), generator=g).to(dtype)
    xs, ws = torch.ones(n, cin // bs, h, w, dtype=dtype), torch.ones(cout, cin // bs, kh, kw, dtype=dtype)
    for t in (x, wt):
        mx_operand.set_format(t, "fp8_e4m3")
    for s in (xs, ws):
        mx_operand.set_pow2(s)
    return dict(input=x, weight=wt, bias=None, stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, input_scale=xs, weight_scale=ws,
                block_size=bs, input_code=None, weight_code=None)


@pytest.fixture
def lifted(monkeypatch):
    """The router with its device test lifted and everything that touches the device replaced, so that CPU tensors reach every later rule."""
    real = mx_gemm._common_ok

    class OnDevice:
        """A CPU tensor that answers "cuda" when asked for its device: everything else of the real predicate stays in force."""
        device = types.SimpleNamespace(type="cuda")

        def __init__(self, t):
            self._t = t

        def __getattr__(self, name):
            return getattr(self._t, name)

    def common_ok(x, scale, code, block_size):
        return real(OnDevice(x), scale, code, block_size)
    rec = _Recorder(0)
    state = {"weight": (0, torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8))}
    monkeypatch.setattr(mx_conv, "_common_ok", common_ok)
    monkeypatch.setattr(mx_conv, "_conv_weight_operand", lambda *a: state["weight"])
    monkeypatch.setattr(mx_conv, "_activation_operand", lambda *a: (torch.zeros(16, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)))
    monkeypatch.setattr(mx_conv, "_stream_ptr", lambda t: None)
    monkeypatch.setattr(mx_conv._native, "lib", lambda: rec)
    monkeypatch.setenv("QT_MX_GEMM", "1")
    mx_gemm.STATS.reset()
    return rec, state


def test_router_takes_the_stand_in_problem(lifted):
    rec, _ = lifted
    y = mx_conv.mx_conv2d_or_none(**_problem())
    assert y is not None and y.shape == (2, 8, 6, 5) and y.dtype == torch.bfloat16 and y.permute(0, 2, 3, 1).is_contiguous()
    assert len(rec.calls) == 1 and rec.calls[0][9:22] == (2, 6, 5, 64, 8, 3, 3, 1, 1, 1, 1, 1, 1)
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 0)


def _with(**kw):
    def change(p, state):
        p.update(kw)
    return change


def _no_format(p, state):
    mx_operand.forget(p["input"])


def _int_format(p, state):
    mx_operand.set_format(p["input"], "int8")


def _not_pow2(which):
    def change(p, state):
        mx_operand.forget(p[which])
    return change


def _scale_shape(which):
    def change(p, state):
        s = p[which][:, :, :-1].contiguous()
        p[which] = mx_operand.set_pow2(s)
    return change


def _weight_refused(p, state):
    state["weight"] = None


def _pair_without_kernel(p, state):
    state["weight"] = (2,) + state["weight"][1:]                    # fp8_e4m3 x fp6_e2m3


def _six_bit_cin_32(p, state):
    q = _problem(cin=32)
    mx_operand.set_format(q["input"], "fp6_e2m3")
    state["weight"] = (2,) + state["weight"][1:]
    p.clear()
    p.update(q)


FALLBACKS = [
    ("groups 2", _with(groups=2)),
    ("no remembered format", _no_format),
    ("a remembered format the instruction does not take", _int_format),
    ("input scale not flagged power-of-two", _not_pow2("input_scale")),
    ("weight scale not flagged power-of-two", _not_pow2("weight_scale")),
    ("block size 64 does not divide Cin = 96", lambda p, s: (p.clear(), p.update(_problem(cin=96, bs=32)), p.update(block_size=64))),
    ("input scale shape", _scale_shape("input_scale")),
    ("weight scale shape", _scale_shape("weight_scale")),
    ("a weight the packer refuses", _weight_refused),
    ("a format pair without a kernel", _pair_without_kernel),
    ("a 6-bit activation with Cin = 32", _six_bit_cin_32),
    ("an empty output", _with(padding=(0, 0), dilation=(3, 3))),
    ("string padding", _with(padding="same")),
]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in FALLBACKS])
def test_router_falls_back_and_counts_it(lifted, change):
    rec, state = lifted
    p = _problem()
    change(p, state)
    assert mx_conv.mx_conv2d_or_none(**p) is None
    assert rec.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)


@pytest.mark.parametrize("k,takes", [(32, False), (64, False), (96, False), (128, True), (192, True), (576, True), (2048, True)])
def test_pack_route_rule(k, takes):
    """profiles/conv2d_mx.txt: a contraction under one 128-deep k tile does not pay for the pack."""
    assert mx_conv._pack_route_takes(k) == takes


def test_rule_declines_only_without_a_packed_operand(lifted):
    rec, _ = lifted
    p = _problem(kh=1, kw=1)                                        # kh kw Cin = 64
    assert mx_conv.mx_conv2d_or_none(**p) is None
    assert rec.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)
    x = p["input"]
    mx_operand.set_operand(x, mx_operand.NHWC, 0, 32, torch.zeros(2 * 6 * 5, 64, dtype=torch.uint8), torch.zeros(2 * 6 * 5, 2, dtype=torch.uint8))
    assert mx_conv.mx_conv2d_or_none(**p) is not None
    assert len(rec.calls) == 1 and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (1, 1)
    mx_operand.set_operand(x, mx_operand.NHWC, 4, *mx_operand.operand_record(x, mx_operand.NHWC)[1:])     # an operand of another format is no operand
    assert mx_conv.mx_conv2d_or_none(**p) is None and len(rec.calls) == 1


@pytest.mark.parametrize("rc", [QT_ERR_BAD_ARG, QT_ERR_UNALIGNED, QT_ERR_BAD_DTYPE])
def test_router_falls_back_when_the_kernel_declines(lifted, rc):
    rec, _ = lifted
    rec.rc = rc
    assert mx_conv.mx_conv2d_or_none(**_problem()) is None
    assert len(rec.calls) == 1 and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 1)


QUIET = [
    ("fp16", lambda p, s: p.update({k: p[k].half() for k in ("input", "weight", "input_scale", "weight_scale")})),
    ("an input codebook", _with(input_code=torch.arange(16.0))),
    ("a weight codebook", _with(weight_code=torch.arange(16.0))),
    ("block size 16", _with(block_size=16)),
    ("block size 48", _with(block_size=48)),
    ("no input scale", _with(input_scale=None)),
    ("operands of two dtypes", lambda p, s: p.update(weight=p["weight"].float(), weight_scale=p["weight_scale"].float())),
]


@pytest.mark.parametrize("change", [pytest.param(c, id=label) for label, c in QUIET])
def test_router_hands_back_what_is_not_a_native_format(lifted, change):
    """What linear_mx / matmul_mx do not count either: the problem never was a candidate."""
    rec, state = lifted
    p = _problem()
    change(p, state)
    assert mx_conv.mx_conv2d_or_none(**p) is None
    assert rec.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


def test_router_is_governed_by_the_gemm_switch(lifted, monkeypatch):
    rec, _ = lifted
    monkeypatch.setenv("QT_MX_GEMM", "0")
    assert mx_conv.mx_conv2d_or_none(**_problem()) is None and rec.calls == []


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    rec = _Recorder(0)
    monkeypatch.setattr(mx_conv._native, "lib", lambda: rec)
    mx_gemm.STATS.reset()
    assert mx_conv.mx_conv2d_or_none(**_problem()) is None
    assert rec.calls == [] and (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


# ---- the composite ---------------------------------------------------------------------------------------------------------------------
def _restated(input, weight, bias, stride, padding, dilation, groups, input_scale, weight_scale, block_size, input_code, weight_code):
    """decomposed.py:289-301, restated: codebook lookup, block scales repeated along the channel axis, F.conv2d."""
    if input_code is not None:
        input = input_code[input.to(torch.long)].to(input.dtype)
    if weight_code is not None:
        weight = weight_code[weight.to(torch.long)].to(weight.dtype)
    if input_scale is not None:
        input = input * torch.repeat_interleave(input_scale, block_size, dim=1)
    if weight_scale is not None:
        weight = weight * torch.repeat_interleave(weight_scale, block_size, dim=1)
    return torch.nn.functional.conv2d(input, weight, bias, stride, padding, dilation, groups)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", ["plain", "strided", "grouped", "codebook", "no scales"])
def test_composite_on_cpu_is_unchanged(case, dtype):
    from quantized_training.fake_quantize import get_quantization_map
    g = torch.Generator().manual_seed(3)
    qmap = get_quantization_map("fp8_e4m3", "cpu")
    groups = 2 if case == "grouped" else 1
    x = (torch.randn(2, 64, 7, 6, generator=g) * 2).to(dtype)
    w = (torch.randn(12, 64 // groups, 3, 2, generator=g) * 0.5).to(dtype)
    bias = torch.randn(12, generator=g).to(dtype)
    xs, xq = torch.ops.quantized_ops.quantize_mx(x, qmap, [1], 32, 448.0, True, None, None)
    ws, wq = torch.ops.quantized_ops.quantize_mx(w, qmap, [1], 32, 448.0, True, None, None)
    kw = dict(input_scale=xs, weight_scale=ws, block_size=32, input_code=None, weight_code=None)
    stride, padding, dilation = ((2, 1), (1, 2), (1, 2)) if case == "strided" else ((1, 1), (1, 1), (1, 1))
    if case == "codebook":
        xq, wq = torch.randint(0, 16, x.shape, generator=g).to(dtype), torch.randint(0, 16, w.shape, generator=g).to(dtype)
        kw.update(input_code=torch.linspace(-3, 3, 16).to(dtype), weight_code=torch.linspace(-1, 1, 16).to(dtype))
    if case == "no scales":
        kw.update(input_scale=None, weight_scale=None)
    mx_gemm.STATS.reset()
    got = torch.ops.quantized_ops.conv2d_mx(xq, wq, bias, stride, padding, dilation, groups, **kw)
    want = _restated(xq, wq, bias, stride, padding, dilation, groups, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert (mx_gemm.STATS.native, mx_gemm.STATS.fallback) == (0, 0)


# ---- the reference's converted CNN -----------------------------------------------------------------------------------------------------
def _generator():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "gen_golden_mx_conv.py")
    spec = importlib.util.spec_from_file_location("gen_golden_mx_conv", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, os.path.dirname(path)


def test_pt2e_block_scaled_cnn_matches_reference():
    """The toy CNN through this package's prepare_pt2e / convert_pt2e on the CPU against what upstream's recorded for the same model,
    inputs and specs (tests/golden/gen_golden_mx_conv.py): graphs row for row, kwargs, node dtypes, buffers and outputs bit for bit."""
    import json
    import os

    import numpy as np

    from quantized_training import quantize_pt2e as qp
    gen, golden = _generator()
    want = json.load(open(os.path.join(golden, "pt2e_mx_conv.json")))
    arr = np.load(os.path.join(golden, "pt2e_mx_conv.npz"))
    arrays, info = gen.record(qp)
    assert info["kw"] == want["kw"]
    assert info["prepared_graph"] == want["prepared_graph"]
    assert info["converted_graph"] == want["converted_graph"]
    assert sum("conv2d_mx" in row[2] for row in info["converted_graph"]) == 3
    assert info["converted_kwargs"] == want["converted_kwargs"]
    assert info["node_dtype"] == want["node_dtype"]
    assert info["buffers"] == want["buffers"]
    assert sorted(arrays) == sorted(arr.files)
    for k in arr.files:
        assert np.array_equal(arrays[k], arr[k]), k
