"""Microscaling along an axis that is not the last, the parts that need no GPU: which calls the strided kernels take
(fake_quantize.mx_block_view), what the four C entry points (qt_quantize_mx_strided_*, qt_fake_quant_mx_strided_*) answer to every
call they decline -- before their first HIP call, so 16-byte-aligned host addresses stand in for device memory --, the graph pass that
folds calculate_mx_qparam + quantize into one quantize_mx node, and the rule that recognises a transposed view."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from quantized_training import _native, fake_quantize as fqz, pt2e_native, quantize_pt2e as qp
from quantized_training._native import QT_ERR_BAD_ARG, QT_ERR_UNALIGNED, QtFormat

G = os.path.join(os.path.dirname(__file__), "golden")
BF16, F32 = torch.bfloat16, torch.float32


# ---- mx_block_view ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype,bs,axes,want", [
    ((2, 3, 64, 40), BF16, 32, -2, (6, 64, 40)),
    ((64, 80), F32, 16, 0, (1, 64, 80)),
    ((2, 24, 8, 16), BF16, 12, 1, (2, 24, 128)),
    ((2, 3, 64, 40), BF16, 32, [-2], (6, 64, 40)),
    ((2, 3, 64, 40), BF16, 32, (-2,), (6, 64, 40)),
    ((2, 3, 64, 40), BF16, 1, 2, (6, 64, 40)),
    ((2, 3, 1024, 8), BF16, 512, 2, (6, 1024, 8)),
])
def test_block_view_takes(shape, dtype, bs, axes, want):
    assert fqz.mx_block_view(shape, dtype, bs, axes) == want


@pytest.mark.parametrize("shape,dtype,bs,axes", [
    pytest.param((2, 3, 64, 40), BF16, 8, -1, id="last axis"),
    pytest.param((2, 3, 64, 40), BF16, 8, 3, id="last axis, counted from the front"),
    pytest.param((2, 3, 64, 40), BF16, 32, (-2, -1), id="two axes"),
    pytest.param((2, 3, 64, 40), BF16, (32,), -2, id="tuple block size"),
    pytest.param((2, 3, 64, 40), BF16, True, -2, id="bool block size"),
    pytest.param((2, 3, 64, 40), torch.float16, 32, -2, id="fp16"),
    pytest.param((2, 3, 64, 36), BF16, 32, -2, id="inner % 8"),
    pytest.param((64, 6), F32, 32, 0, id="inner % 4"),
    pytest.param((2, 3, 64, 40), BF16, 24, -2, id="n % bs"),
    pytest.param((2, 3, 64, 40), BF16, 0, -2, id="bs 0"),
    pytest.param((2, 3, 1026, 40), BF16, 513, -2, id="bs 513"),
    pytest.param((2, 0, 64, 40), BF16, 32, -2, id="empty"),
    pytest.param((2, 3, 64, 40), BF16, 32, 4, id="axis out of range"),
    pytest.param((64,), BF16, 32, 0, id="one dimension"),
    pytest.param((64, 1), BF16, 32, 0, id="inner 1"),
])
def test_block_view_refuses(shape, dtype, bs, axes):
    assert fqz.mx_block_view(shape, dtype, bs, axes) is None


# ---- declines of the C ABI ----------------------------------------------------------------------------------------------------------
_BUF = ctypes.create_string_buffer(4096 + 64)
P = (ctypes.addressof(_BUF) + 63) & ~63              # stands in for every device pointer
OFF = P + 8                                          # off a 16-byte boundary
LUT = QtFormat(_native.QT_FMT_LUT, 0, 0, 0.0, 0.0)
HUGE = (2 ** 32) * 8                                  # inner / 8 (and / 4) above 2^32 - 1


def _quantize(L, io, **kw):
    a = dict(x=P, q=P, s=P, codes=None, e8=None, outer=2, n=64, inner=32, bs=32, fmt=LUT, lut=P, qmax=448.0, pow2=1, smap=None, pf=0)
    a.update(kw)
    fn = getattr(L, f"qt_quantize_mx_strided_{io}")
    return fn(a["x"], a["q"], a["s"], a["codes"], a["e8"], a["outer"], a["n"], a["inner"], a["bs"],
              ctypes.byref(a["fmt"]) if a["fmt"] is not None else None, a["lut"], a["qmax"], a["pow2"], a["smap"], a["pf"], None)


def _fake_quant(L, io, **kw):
    a = dict(x=P, q=P, s=P, outer=2, n=64, inner=32, bs=32, fmt=LUT, lut=P, qmax=448.0, pow2=0, smap=None)
    a.update(kw)
    fn = getattr(L, f"qt_fake_quant_mx_strided_{io}")
    return fn(a["x"], a["q"], a["s"], a["outer"], a["n"], a["inner"], a["bs"], ctypes.byref(a["fmt"]) if a["fmt"] is not None else None,
              a["lut"], a["qmax"], a["pow2"], a["smap"], None)


# what both families decline
COMMON = [
    ("NULL x", dict(x=None), QT_ERR_BAD_ARG),
    ("NULL scales", dict(s=None), QT_ERR_BAD_ARG),
    ("NULL fmt", dict(fmt=None), QT_ERR_BAD_ARG),
    ("table format without a table", dict(lut=None), QT_ERR_BAD_ARG),
    ("block size 0", dict(bs=0, n=64), QT_ERR_BAD_ARG),
    ("block size 513", dict(bs=513, n=1026), QT_ERR_BAD_ARG),
    ("quant_max 0", dict(qmax=0.0), QT_ERR_BAD_ARG),
    ("quant_max negative", dict(qmax=-1.0), QT_ERR_BAD_ARG),
    ("inner 1", dict(inner=1), QT_ERR_BAD_ARG),
    ("inner above 2^32 - 1 vectors", dict(inner=HUGE), QT_ERR_BAD_ARG),
    ("n % block_size", dict(n=72), QT_ERR_UNALIGNED),
    ("inner off the vector", dict(inner=34), QT_ERR_UNALIGNED),
    ("x off 16 bytes", dict(x=OFF), QT_ERR_UNALIGNED),
    ("q off 16 bytes", dict(q=OFF), QT_ERR_UNALIGNED),
    ("scales off 16 bytes", dict(s=OFF), QT_ERR_UNALIGNED),
]
# the packed operand
PACK = dict(codes=P, e8=P)
PACKED = [
    ("codes without e8m0", dict(codes=P), QT_ERR_BAD_ARG),
    ("e8m0 without codes", dict(e8=P), QT_ERR_BAD_ARG),
    ("pack without force_pow2", dict(PACK, pow2=0), QT_ERR_BAD_ARG),
    ("pack_format -1", dict(PACK, pf=-1), QT_ERR_BAD_ARG),
    ("pack_format 5", dict(PACK, pf=5), QT_ERR_BAD_ARG),
    ("pack with block size 16", dict(PACK, bs=16), QT_ERR_BAD_ARG),
    ("pack with block size 48", dict(PACK, bs=48, n=96), QT_ERR_BAD_ARG),
    ("codes off 16 bytes", dict(PACK, codes=OFF), QT_ERR_UNALIGNED),
    ("e8m0 off 16 bytes", dict(PACK, e8=OFF), QT_ERR_UNALIGNED),
    # n bits / 8 off 16 bytes: only the 6-bit formats can miss it when n is a multiple of 32 (24 bytes per 32 elements)
    ("code row of 24 bytes", dict(PACK, n=32, bs=32, pf=2), QT_ERR_UNALIGNED),
    ("code row of 72 bytes", dict(PACK, n=96, bs=32, pf=3), QT_ERR_UNALIGNED),
]

CASES = [pytest.param(_quantize, io, kw, code, id=f"quantize_{io}-{label}") for io in ("bf16", "f32") for label, kw, code in COMMON + PACKED]
CASES += [pytest.param(_fake_quant, io, kw, code, id=f"fake_quant_{io}-{label}") for io in ("bf16", "f32") for label, kw, code in COMMON]
CASES += [pytest.param(_fake_quant, io, dict(q=None), QT_ERR_BAD_ARG, id=f"fake_quant_{io}-NULL y") for io in ("bf16", "f32")]


@pytest.mark.parametrize("call,io,kw,code", CASES)
def test_declines_before_the_first_hip_call(call, io, kw, code):
    assert call(_native.lib(), io, **kw) == code


@pytest.mark.parametrize("call", [_quantize, _fake_quant])
@pytest.mark.parametrize("io", ["bf16", "f32"])
@pytest.mark.parametrize("empty", [dict(outer=0), dict(n=0), dict(inner=0)])
def test_empty_tensor_is_ok_without_a_launch(call, io, empty):
    assert call(_native.lib(), io, **empty) == 0


# ---- fuse_mx_pairs on the golden toy ------------------------------------------------------------------------------------------------
def _converted(name, native):
    import test_pt2e_cpu as t
    arr = np.load(os.path.join(G, "pt2e_mx.npz"))
    info, m, xs = t.mx_setup(name, arr)
    gm = qp.prepare_pt2e(m, qp.get_default_quantizer(**info["kw"]), (xs[0],))
    with torch.no_grad():
        gm(xs[0])
        gm(xs[1])
    return info, arr, xs, qp.convert_pt2e(gm, native=native), t


def _activation_qparam_nodes(gc):
    return [n for n in gc.graph.nodes if n.op == "call_function" and n.target == torch.ops.quantized_ops.calculate_mx_qparam.default
            and n.args[0].op != "get_attr"]


def _pairs(gc):
    """(calculate_mx_qparam, quantize) pairs of an activation in an unfolded graph, counted the way the issue states the rule."""
    Q, C = torch.ops.quantized_ops.quantize.default, torch.ops.quantized_ops.calculate_mx_qparam.default
    mx = (torch.ops.quantized_ops.linear_mx.default, torch.ops.quantized_ops.matmul_mx.default, torch.ops.quantized_ops.conv2d_mx.default)
    n = 0
    for q in gc.graph.nodes:
        if q.op != "call_function" or q.target != Q:
            continue
        s = q.args[1]
        if not (isinstance(s, torch.fx.Node) and s.op == "call_function" and s.target == C):
            continue
        if s.args[0] is not q.args[0] or s.args[0].op == "get_attr" or q.args[2] is not None or (len(q.args) > 6 and q.args[6] is not None):
            continue
        if list(s.args[1]) != list(q.args[3]) or s.args[2] != q.args[4]:
            continue
        if all(u is q or u.target in mx for u in s.users):
            n += 1
    return n


MX_CONFIGS = sorted(json.load(open(os.path.join(G, "pt2e_mx.json"))))


@pytest.mark.parametrize("name", MX_CONFIGS)
def test_fold_on_the_golden_toy(name):
    assert len(MX_CONFIGS) == 5                                      # every configuration of the golden
    info, arr, xs, plain, t = _converted(name, native=False)
    assert t._rows(plain) == info["converted_graph"]                 # native=False: upstream's graph, node for node
    pairs = _pairs(plain)
    assert pairs >= 1
    assert pt2e_native.fuse_mx_pairs(plain) == pairs                 # the pass itself reports what it folded
    assert pt2e_native.fuse_mx_pairs(plain) == 0                     # and is idempotent

    info, arr, xs, gc, t = _converted(name, native=True)
    assert _activation_qparam_nodes(gc) == []
    mx = [n for n in gc.graph.nodes if n.op == "call_function" and n.target == torch.ops.quantized_ops.quantize_mx.default
          and tuple(n.args[2]) == (-2,)]
    assert len(mx) >= 1
    for n in mx:
        assert isinstance(n.meta["dtype"], tuple) and len(n.meta["dtype"]) == 2
        users = sorted(u.args[1] for u in n.users)
        assert users == [0, 1]
    with torch.no_grad():
        y = gc(xs[1])
    assert np.array_equal(t._bits(y), arr[f"{name}__y_converted"])  # the reference's own recorded output, bit for bit


def _hand_built(s_axes, q_axes):
    """x -> calculate_mx_qparam(x, s_axes, 32, 448, True) + quantize(x, s, None, q_axes, 32, qmap) -> matmul_mx(a, q, weight_scale=s)"""
    ops = torch.ops.quantized_ops
    root = torch.nn.Module()
    root.register_buffer("qmap", fqz.get_quantization_map("fp8_e4m3", "cpu").clone())
    g = torch.fx.Graph()
    a, x = g.placeholder("a"), g.placeholder("x")
    m = g.get_attr("qmap")
    s = g.call_function(ops.calculate_mx_qparam.default, (x, s_axes, 32, 448.0, True))
    q = g.call_function(ops.quantize.default, (x, s, None, q_axes, 32, m, None))
    g.output(g.call_function(ops.matmul_mx.default, (a, q), {"weight_scale": s, "block_size": 32}))
    return torch.fx.GraphModule(root, g)


def test_fold_takes_bare_int_axes_and_skips_what_it_cannot_compare():
    a, x = torch.randn(4, 64), torch.randn(64, 16)
    want = _hand_built([-2], [-2])(a, x)
    gm = _hand_built(-2, [-2])                                              # (the operator itself wants a list: only the fold can run it)
    assert pt2e_native.fuse_mx_pairs(gm) == 1
    mx = [n for n in gm.graph.nodes if n.op == "call_function" and n.target == torch.ops.quantized_ops.quantize_mx.default]
    assert len(mx) == 1 and list(mx[0].args[2]) == [-2]
    assert torch.equal(gm(a, x), want)
    assert pt2e_native.fuse_mx_pairs(_hand_built([-2], [-1])) == 0          # different axes
    assert pt2e_native.fuse_mx_pairs(_hand_built([-2], None)) == 0          # quantize without axes
    assert pt2e_native.fuse_mx_pairs(_hand_built("rows", "rows")) == 0      # nothing the pass can compare: skipped, not raised


# ---- transposed views ---------------------------------------------------------------------------------------------------------------------
def test_transposed_view_rule():
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    v = t.transpose(-1, -2)
    s = fqz.transposed_storage(v)
    assert s is not None and s.data_ptr() == t.data_ptr() and s.shape == t.shape and s.is_contiguous()
    assert fqz.transposed_storage(t) is None                               # contiguous
    assert fqz.transposed_storage(t[..., 1:]) is None                      # a slice
    assert fqz.transposed_storage(t[..., 1:].transpose(-1, -2)) is None    # the transpose of a slice
    assert fqz.transposed_storage(torch.arange(8.0)) is None               # one dimension
    assert fqz.transposed_storage(torch.arange(8.0)[::2]) is None
