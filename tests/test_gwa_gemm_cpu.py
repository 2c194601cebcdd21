"""Packed group-wise affine weights without a GPU: the C ABI's new entry points, the packed layout in torch ops, and the graph pass
fuse_gwa_linears (pt2e_native.py) -- what it rewrites, bit for bit against the unfused graph, and every case it must leave alone."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

from quantized_training import _native, pt2e_native
from quantized_training import quantize_pt2e as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["qt_gwa_packed_bytes", "qt_gwa_pack", "qt_gwa_dequantize_bf16", "qt_linear_gwa_tile", "qt_linear_gwa_bf16"]
DQ, LIN = "quantized_ops.dequantize.default", "aten.linear.default"
GWA = "quantized_ops.linear_gwa.default"


@pytest.fixture(autouse=True)
def _leave_no_routes():
    """routes_report() of later tests lists what THEY ran: the process-wide table of linear_gwa routes is put back as this test found it."""
    before = dict(pt2e_native.GWA_ROUTES)
    yield
    pt2e_native.GWA_ROUTES.clear()
    pt2e_native.GWA_ROUTES.update(before)


# ---- symbols and signatures -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    assert "#define QT_ABI_VERSION 3" in header and _native.ABI_VERSION == 3
    cdll = ctypes.CDLL(_native.LIB_PATH)
    assert cdll.qt_abi_version() == 3
    for name in ENTRY_POINTS:
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl is not None, name
        assert name in _native.SIGNATURES, name
        n_args = len([a for a in decl.group(1).split(",") if a.strip()])
        assert n_args == len(_native.SIGNATURES[name][1]), name
        getattr(cdll, name)


def test_host_side_answers_need_no_device():
    L = _native.lib()
    assert L.qt_gwa_packed_bytes(16, 128, 4) == 1024 and L.qt_gwa_packed_bytes(16, 64, 8) == 1024
    assert L.qt_gwa_packed_bytes(24, 160, 4) == 2 * 2 * 1024          # columns round up to 16, k to the super step
    assert L.qt_gwa_packed_bytes(16, 128, 5) == 0 and L.qt_gwa_packed_bytes(12, 128, 4) == 0 and L.qt_gwa_packed_bytes(16, 48, 4) == 0
    assert [L.qt_linear_gwa_tile(m) for m in (1, 16, 17, 32, 33, 64, 65, 4096)] == [16, 16, 32, 32, 64, 64, 64, 64]
    # declines are answered before any device call: they work on a box without a GPU
    one = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(one)
    p += (-p) % 16
    assert L.qt_linear_gwa_bf16(None, p, p, p, None, p, 1, 16, 128, 128, 4, 0.0, 0, None) == _native.QT_ERR_BAD_ARG
    assert L.qt_linear_gwa_bf16(p, p, p, p, None, p, 1, 16, 128, 128, 3, 0.0, 0, None) == _native.QT_ERR_BAD_ARG
    assert L.qt_linear_gwa_bf16(p, p, p, p, None, p, 1, 16, 128, 48, 4, 0.0, 0, None) == _native.QT_ERR_BAD_ARG
    assert L.qt_linear_gwa_bf16(p, p, p, p, None, p, 1, 16, 128, 128, 4, 0.0, 48, None) == _native.QT_ERR_BAD_ARG
    assert L.qt_linear_gwa_bf16(p, p, p, p, None, p, 1, 16, 192, 128, 4, 0.0, 0, None) == _native.QT_ERR_UNALIGNED
    assert L.qt_linear_gwa_bf16(p, p, p, p, None, p, 1, 12, 128, 128, 4, 0.0, 0, None) == _native.QT_ERR_UNALIGNED
    assert L.qt_linear_gwa_bf16(p + 2, p, p, p, None, p, 1, 16, 128, 128, 4, 0.0, 0, None) == _native.QT_ERR_UNALIGNED
    assert L.qt_gwa_pack(p, p, 16, 128, 4, 0.0, 16.0, None, None) == _native.QT_ERR_BAD_ARG          # 17 codes in 4 bits
    assert L.qt_gwa_dequantize_bf16(p, p, p, None, 16, 128, 128, 4, 0.0, None) == _native.QT_ERR_BAD_ARG


# ---- pack -> unpack in torch ops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,N,K", [(4, 16, 128), (4, 24, 96), (4, 8, 32), (4, 40, 416), (8, 16, 64), (8, 24, 96), (8, 8, 32), (8, 264, 160)])
def test_pack_unpack_round_trip_over_all_code_values(bits, N, K):
    span = 16 if bits == 4 else 256
    qmin = -8 if bits == 4 else -128
    g = torch.Generator().manual_seed(N * K + bits)
    codes = torch.randint(0, span, (N, K), generator=g)
    codes.view(-1)[:span] = torch.arange(span)                               # every code value at least once
    packed = pt2e_native.gwa_pack_torch((codes + qmin).to(torch.bfloat16), qmin, qmin + span - 1, bits)
    assert packed.dtype == torch.uint8 and packed.numel() == _native.lib().qt_gwa_packed_bytes(N, K, bits)
    assert torch.equal(pt2e_native.gwa_unpack_torch(packed, N, K, bits).long(), codes)


def test_layout_is_the_documented_one():
    """include/qt_hip.h: the piece of lane 16 g + r of (group, super step) holds column 16 group + r, k = base + 32 j + 8 g + e."""
    N, K = 32, 256
    codes = (torch.arange(N * K).view(N, K) * 7 + torch.arange(N).view(N, 1)) % 16
    p = pt2e_native.gwa_pack_torch(codes.to(torch.bfloat16), 0, 15, 4)
    for (ng, ss, g, r, j, e) in [(0, 0, 0, 0, 0, 0), (1, 1, 3, 15, 3, 7), (1, 0, 2, 5, 1, 4), (0, 1, 1, 9, 2, 3)]:
        byte = int(p[((ng * 2 + ss) * 64 + 16 * g + r) * 16 + 4 * j + e // 2])
        assert (byte >> (4 * (e & 1))) & 15 == int(codes[16 * ng + r, ss * 128 + 32 * j + 8 * g + e])
    codes8 = (torch.arange(N * K).view(N, K) * 37) % 256
    p = pt2e_native.gwa_pack_torch(codes8.to(torch.bfloat16), 0, 255, 8)
    for (ng, ss, g, r, j, e) in [(0, 0, 0, 0, 0, 0), (1, 3, 3, 15, 1, 7), (1, 2, 2, 5, 1, 4)]:
        assert int(p[((ng * 4 + ss) * 64 + 16 * g + r) * 16 + 8 * j + e]) == int(codes8[16 * ng + r, ss * 64 + 32 * j + 8 * g + e])


@pytest.mark.parametrize("bad", [0.5, 16.0, -1.0, float("nan")])
def test_torch_packer_refuses_a_bad_code(bad):
    codes = torch.zeros(16, 128, dtype=torch.bfloat16)
    assert pt2e_native.gwa_pack_torch(codes, 0, 15, 4) is not None
    codes[3, 77] = bad
    assert pt2e_native.gwa_pack_torch(codes, 0, 15, 4) is None


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------
class TwoLinears(nn.Module):
    def __init__(self, k=64, h=64, n=24):
        super().__init__()
        self.fc1 = nn.Linear(k, h)
        self.fc2 = nn.Linear(h, n, bias=False)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


def prepared(spec, model, x, object_type=torch.ops.aten.linear.default):
    from quantized_training.fake_quantize import FusedAmaxObsFakeQuantize
    from quantized_training.quantizer.quantizer import QuantizationSpec
    from quantized_training.quantizer.xnnpack_quantizer import XNNPACKQuantizer
    from quantized_training.quantizer.xnnpack_quantizer_utils import QuantizationConfig
    w = QuantizationSpec.from_str(spec)
    w.observer_or_fake_quant_ctr = FusedAmaxObsFakeQuantize
    q = XNNPACKQuantizer().set_object_type(object_type, QuantizationConfig(None, None, w, None))
    gm = qp.prepare_pt2e(model, q, (x,))
    with torch.no_grad():
        gm(x)
    return gm


def both(spec, dtype=torch.bfloat16, make=TwoLinears, x_shape=(3, 64)):
    """(unfused, fused-if-possible) conversions of the same prepared model, and an input."""
    out = []
    for native in (False, True):
        torch.manual_seed(0)
        m = make().eval().to(dtype)
        x = torch.randn(*x_shape).to(dtype)
        out.append(qp.convert_pt2e(prepared(spec, m, x), native=native))
    return out[0], out[1], x


def rows(gm):
    return [(n.op, str(n.target), tuple(str(a) for a in n.args), n.name) for n in gm.graph.nodes]


def targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


FORMATS = ["uint4,qs=group_wise_affine,bs=32,ax=-1", "int4,qs=group_wise_affine,bs=32,ax=-1", "uint2,qs=group_wise_affine,bs=32,ax=-1",
           "uint8,qs=group_wise_affine,bs=32,ax=-1", "uint4,qs=group_wise_affine,bs=32,ax=-1,scale=fp8_e5m3",
           "uint4,qs=group_wise_affine,bs=64,ax=-1"]


@pytest.mark.parametrize("spec", FORMATS, ids=[f.split(",")[0] + ("-e5m3" if "scale=" in f else "") + "-" + f.split("bs=")[1][:2] for f in FORMATS])
def test_pass_packs_the_weight_and_keeps_every_bit(spec):
    plain, fused, x = both(spec)
    dtype = spec.split(",")[0]
    assert targets(plain).count(DQ) == 2 and targets(plain).count(LIN) == 2
    assert targets(fused).count(GWA) == 2 and DQ not in targets(fused) and LIN not in targets(fused)
    bufs = dict(fused.named_buffers())
    packed = {k: v for k, v in bufs.items() if k.endswith("_packed")}
    assert len(packed) == 2 and all(v.dtype == torch.uint8 for v in packed.values())
    assert not any(k.endswith("_" + dtype) for k in bufs), sorted(bufs)         # the bf16 codes are gone ...
    assert any(k.endswith("_" + dtype) for k in dict(plain.named_buffers()))
    bits = pt2e_native.gwa_dtype_range(dtype)[2]
    for k, v in packed.items():                                                 # ... and 16 bits per weight became 4 or 8
        codes = dict(plain.named_buffers())[k[:-len("_packed")]]
        assert v.numel() == _native.lib().qt_gwa_packed_bytes(codes.shape[0], codes.shape[1], bits)
    assert set(fused.state_dict()) >= set(packed)                               # persistent: the packed weight is the checkpoint
    with torch.no_grad():
        assert torch.equal(plain(x), fused(x))
    node = next(n for n in fused.graph.nodes if str(n.target) == GWA)
    lo = pt2e_native.gwa_dtype_range(dtype)[0]
    assert node.args[5:] == (int(spec.split("bs=")[1].split(",")[0]), lo, bits, 64)


def test_pass_is_idempotent_and_reports_its_count():
    _, fused, _ = both(FORMATS[0])
    before = rows(fused)
    assert pt2e_native.fuse_gwa_linears(fused) == 0
    assert rows(fused) == before


def test_default_conversion_of_a_cpu_model_is_upstreams_graph():
    torch.manual_seed(0)
    m = TwoLinears().eval().bfloat16()
    x = torch.randn(3, 64).bfloat16()
    default = qp.convert_pt2e(prepared(FORMATS[0], m, x))
    plain, _, _ = both(FORMATS[0])
    assert rows(default) == rows(plain)
    assert {k: v.dtype for k, v in default.named_buffers()} == {k: v.dtype for k, v in plain.named_buffers()}


def assert_declined(plain, fused, x=None):
    assert rows(fused) == rows(plain)
    assert GWA not in targets(fused)
    a, b = dict(plain.named_buffers()), dict(fused.named_buffers())
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) or (a[k] != a[k]).any() for k in a)
    if x is not None:
        with torch.no_grad():
            assert torch.equal(plain(x), fused(x), ) or bool((plain(x) != plain(x)).any())


def hand_edit(edit, spec=FORMATS[0]):
    """The unfused conversion twice, `edit` applied to both, the pass applied to the second."""
    plain, _, x = both(spec)
    other, _, _ = both(spec)
    for gm in (plain, other):
        edit(gm)
        gm.graph.lint()
        gm.recompile()
    assert rows(plain) == rows(other)
    n = pt2e_native.fuse_gwa_linears(other)
    return plain, other, x, n


def dq_nodes(gm):
    return [n for n in gm.graph.nodes if str(n.target) == DQ]


def test_declines_fp32_and_fp16_models():
    for dtype in (torch.float32, torch.float16):
        plain, fused, x = both(FORMATS[0], dtype=dtype)
        assert_declined(plain, fused, x)


def test_declines_blocks_along_the_first_axis():
    plain, fused, x = both("uint4,qs=group_wise_affine,bs=8,ax=0")
    assert targets(plain).count(DQ) == 2
    assert_declined(plain, fused, x)


def test_declines_a_tuple_block_size():
    def tuple_blocks(gm):                                     # what a `bs=(1,32),ax=(0,1)` spec lowers to
        for dq in dq_nodes(gm):
            dq.args = tuple(dq.args[:3]) + ((0, 1), (1, 32))
    plain, other, x, n = hand_edit(tuple_blocks)
    assert n == 0
    assert_declined(plain, other)                             # (the op's schema takes an int: such a graph is compared, not run)


def test_declines_a_block_size_the_kernels_do_not_take():
    plain, fused, x = both("uint4,qs=group_wise_affine,bs=16,ax=-1")
    assert_declined(plain, fused, x)


class ConvNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(32, 16, 1)

    def forward(self, x):
        return self.conv(x)


def test_declines_a_conv_weight():
    out = []
    for native in (False, True):
        torch.manual_seed(0)
        m = ConvNet().eval().bfloat16()
        x = torch.randn(2, 32, 4, 4).bfloat16()
        gm = prepared("uint4,qs=group_wise_affine,bs=32,ax=1", m, x, object_type=torch.ops.aten.conv2d.default)
        out.append(qp.convert_pt2e(gm, native=native))
    assert targets(out[0]).count(DQ) == 1
    assert_declined(out[0], out[1], x)


def test_declines_a_shared_dequantize():
    def share(gm):
        dq = dq_nodes(gm)[0]
        lin = next(iter(dq.users))
        with gm.graph.inserting_after(lin):
            extra = gm.graph.call_function(torch.ops.aten.sum.default, (dq,))
        out = next(n for n in gm.graph.nodes if n.op == "output")
        with gm.graph.inserting_before(out):
            add = gm.graph.call_function(torch.ops.aten.add.Tensor, (out.args[0][0] if isinstance(out.args[0], (tuple, list)) else out.args[0], extra))
        out.args = ((add,),) if isinstance(out.args[0], (tuple, list)) else (add,)
    plain, other, x, n = hand_edit(share)
    assert n == 1                                                               # the other Linear is still fused
    assert targets(other).count(DQ) == 1 and targets(other).count(GWA) == 1
    shared = dq_nodes(other)[0]
    assert len(shared.users) == 2 and str(shared.args[0].target) in dict(other.named_buffers())
    with torch.no_grad():
        assert torch.equal(plain(x), other(x))


def test_declines_an_output_qmap():
    def add_map(gm):
        import quantized_training as qt
        gm.register_buffer("out_map", qt.get_quantization_map("fp8_e4m3", torch.device("cpu")))
        for dq in dq_nodes(gm):
            with gm.graph.inserting_before(dq):
                m = gm.graph.create_node("get_attr", "out_map")
            dq.args = tuple(dq.args) + (None, m)
    plain, other, x, n = hand_edit(add_map)
    assert n == 0
    assert_declined(plain, other, x)


@pytest.mark.parametrize("bad", [0.5, 16.0, -1.0, float("nan")], ids=["fraction", "above", "below", "nan"])
def test_declines_codes_that_fail_the_packers_check(bad):
    def plant(gm):
        q = dq_nodes(gm)[0].args[0]
        gm.get_buffer(q.target)[5, 9] = bad
    plain, other, x, n = hand_edit(plant)
    assert n == 1                                                               # only the planted weight stays a value tensor
    kept = dq_nodes(other)
    assert len(kept) == 1 and str(kept[0].args[0].target) == str(dq_nodes(plain)[0].args[0].target)
    assert str(next(iter(kept[0].users)).target) == LIN
    assert not any(k.startswith(str(kept[0].args[0].target)) and k.endswith("_packed") for k in dict(other.named_buffers()))
    with torch.no_grad():
        a, b = plain(x), other(x)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) or torch.equal(torch.isnan(a), torch.isnan(b))


def test_operator_has_a_meta_kernel_and_the_reference_route_counts():
    _, fused, x = both(FORMATS[0])
    node = next(n for n in fused.graph.nodes if str(n.target) == GWA)
    packed, scale, zero = (fused.get_buffer(a.target) for a in node.args[1:4])
    y = torch.ops.quantized_ops.linear_gwa(x.to("meta"), packed.to("meta"), scale.to("meta"), zero.to("meta"), None, *node.args[5:])
    assert y.device.type == "meta" and tuple(y.shape) == (3, scale.shape[0]) and y.dtype == torch.bfloat16
    pt2e_native.GWA_STATS.reset()
    with torch.no_grad():
        fused(x)
    assert (pt2e_native.GWA_STATS.fused, pt2e_native.GWA_STATS.dequant, pt2e_native.GWA_STATS.reference) == (0, 0, 2)
    from quantized_training import fused as fz
    assert fz.routes_report().get("gwa:3x24x64") == "unpack+dequantize+linear"
