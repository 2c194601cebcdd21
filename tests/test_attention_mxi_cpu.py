"""The block-scaled integer attention core off the GPU: the symbol, the graph pass (pt2e_native.fuse_mx_attention) on a hand-built
converted graph and behind convert_pt2e on an exported toy, the operator on CPU tensors (the replaced nodes, bit for bit) and the
committed route rule."""
import operator
import os

import pytest
import torch

import quantized_training  # noqa: F401
from quantized_training import _native, mx_attention, pt2e_native
from quantized_training import quantize_pt2e as qp
from quantized_training.fake_quantize import get_quantization_map

OPS, ATEN = torch.ops.quantized_ops, torch.ops.aten
BF16 = torch.bfloat16


def toy_graph(layers=2, D=64, scaling=0.125, div=False, variant=None):
    """x [B, H, S, D], mask -> self-attention layers as a converted block-scaled graph holds them (int6, block 64, fp8_e5m3 scales);
    returns every layer's output.  `variant` breaks the pattern: second_user | dropout | dim | tensor_scale."""
    root = torch.nn.Module()
    root.register_buffer("qmap", get_quantization_map("int6").clone())
    root.register_buffer("smap", get_quantization_map("fp8_e5m3").clone())
    root.register_buffer("c", torch.tensor(scaling, dtype=BF16))
    for name in ("qmap", "smap"):
        quantized_training.mx_operand.copy_hints(get_quantization_map("int6" if name == "qmap" else "fp8_e5m3"), getattr(root, name))
    g = torch.fx.Graph()
    x, mask = g.placeholder("x"), g.placeholder("mask")
    qmap, smap = g.get_attr("qmap"), g.get_attr("smap")

    def qmx(t, axis):
        mx = g.call_function(OPS.quantize_mx.default, (t, qmap, [axis], 64, 31.0, False, smap, None))
        return g.call_function(operator.getitem, (mx, 0)), g.call_function(operator.getitem, (mx, 1))

    outs = []
    for _ in range(layers):
        qs, qq = qmx(x, -1)
        ks, kq = qmx(g.call_function(ATEN.transpose.int, (x, -1, -2)), -2)
        vs, vq = qmx(x, -2)
        s = g.call_function(OPS.matmul_mx.default, (qq, kq), {"input_scale": qs, "weight_scale": ks, "block_size": 64})
        factor = g.get_attr("c") if variant == "tensor_scale" else scaling
        s = g.call_function(ATEN.div.Tensor if div else ATEN.mul.Tensor, (s, factor))
        s = g.call_function(ATEN.add.Tensor, (s, mask))
        p = g.call_function(ATEN.softmax.int, (s, -2 if variant == "dim" else -1))
        if variant == "second_user":
            outs.append(p)
        if variant == "dropout":
            p = g.call_function(ATEN.dropout.default, (p, 0.1, True))
        ps, pq = qmx(p, -1)
        x = g.call_function(OPS.matmul_mx.default, (pq, vq), {"input_scale": ps, "weight_scale": vs, "block_size": 64})
        outs.append(x)
    g.output(tuple(outs))
    return torch.fx.GraphModule(root, g)


def targets(gm):
    return [n.target for n in gm.graph.nodes if n.op == "call_function"]


def test_symbol_in_library_and_header():
    assert "qt_attention_mxi" in _native.SIGNATURES and getattr(_native.lib(), "qt_attention_mxi")
    header = os.path.join(os.path.dirname(__file__), "..", "include", "qt_hip.h")
    assert "int qt_attention_mxi(" in open(header).read()
    assert _native.lib().qt_abi_version() == 3


@pytest.mark.parametrize("div", [False, True])
def test_pass_rewrites_the_span_node_by_node(div):
    gm = toy_graph(layers=2, div=div)
    torch.manual_seed(0)
    x = torch.randn(1, 2, 64, 64).to(BF16)
    mask = torch.zeros(1, 1, 64, 64, dtype=BF16).masked_fill(torch.ones(64, 64).triu(1).bool(), float("-inf"))
    before = gm(x, mask)
    assert pt2e_native.fuse_mx_attention(gm) == 2
    t = targets(gm)
    assert t.count(OPS.attention_mx.default) == 2 and OPS.matmul_mx.default not in t and ATEN.softmax.int not in t
    assert t.count(OPS.quantize_mx.default) == 6                        # q, k^T and v of each layer stay; P's is folded
    for node in gm.graph.nodes:
        if node.target == OPS.attention_mx.default:
            q, qs, kT, ks, v, vs, m, c, is_div, qmap, qmax, pow2, smap, in_f32, bs = node.args[:15]
            assert [n.args[1] for n in (q, qs, kT, ks, v, vs)] == [1, 0, 1, 0, 1, 0] and q.args[0] is qs.args[0]
            assert kT.args[0].args[0].target == ATEN.transpose.int and m.op == "placeholder"
            assert (c, is_div, qmax, pow2, in_f32, bs) == (0.125, div, 31.0, False, False, 64)
            assert (qmap.target, smap.target) == ("qmap", "smap")
    assert pt2e_native.fuse_mx_attention(gm) == 0                       # idempotent
    after = gm(x, mask)                                                 # CPU tensors: the operator runs the replaced nodes
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(after, before))
    meta = OPS.attention_mx(*(torch.empty(s, dtype=BF16, device="meta") for s in
                              ((1, 2, 8, 64), (1, 2, 8, 1), (1, 2, 64, 64), (1, 2, 1, 64), (1, 2, 64, 64), (1, 2, 1, 64))),
                            None, 1.0, False, torch.empty(65536, dtype=BF16, device="meta"), 31.0, False, None, False, 64)
    assert meta.shape == (1, 2, 8, 64)


@pytest.mark.parametrize("variant", ["second_user", "dropout", "dim", "tensor_scale"])
def test_pass_leaves_other_patterns_alone(variant):
    gm = toy_graph(layers=1, variant=variant)
    code = gm.code
    assert pt2e_native.fuse_mx_attention(gm) == 0 and gm.code == code


class ToyAttention(torch.nn.Module):
    """Two self-attention layers on x [B, H, S, 64] under an additive mask; every layer's output."""
    def forward(self, x, mask):
        outs = []
        for _ in range(2):
            a = torch.matmul(x, x.transpose(-1, -2)) * 0.125 + mask
            x = torch.matmul(torch.softmax(a, -1), x)
            outs.append(x)
        return tuple(outs)


def converted_toy(x, mask, **convert_kw):
    """ToyAttention exported, prepared with the recipe's matmul quantizers (int6, block 64, fp8_e5m3 scales), calibrated and converted."""
    spec = "int6,qs=microscaling,bs=64,ax=-1,scale=fp8_e5m3"
    gm = qp.prepare_pt2e(ToyAttention().eval(), qp.get_default_quantizer(spec, weight=spec), (x, mask)).to(x.device)
    with torch.no_grad():
        gm(x, mask)
    return qp.convert_pt2e(gm, native=True, **convert_kw)


def test_convert_folds_only_when_asked():
    torch.manual_seed(1)
    x = torch.randn(1, 2, 64, 64).to(BF16)
    mask = torch.zeros(1, 1, 64, 64, dtype=BF16).masked_fill(torch.ones(64, 64).triu(1).bool(), float("-inf"))
    default, off, on = converted_toy(x, mask), converted_toy(x, mask, fuse_attention=False), converted_toy(x, mask, fuse_attention=True)
    assert default.code == off.code and OPS.attention_mx.default not in targets(off)         # today's graph, node for node
    assert sorted(dict(default.named_buffers())) == sorted(dict(off.named_buffers())) == sorted(dict(on.named_buffers()))
    t = targets(on)
    assert t.count(OPS.attention_mx.default) == 2 and OPS.matmul_mx.default not in t and t.count(OPS.quantize_mx.default) == 6
    assert [n.args[7:9] for n in on.graph.nodes if n.target == OPS.attention_mx.default] == [(0.125, False)] * 2   # export's lifted constant
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(on(x, mask), off(x, mask)))


def test_route_rule_is_the_committed_table():
    assert len(mx_attention._MXI_ATTENTION_TABLE) == 6                 # the classes profiles/attention_mxi.txt shows clearing the bar
    for shape, takes in mx_attention._MXI_ATTENTION_TABLE.items():
        assert takes is True and mx_attention._mxi_attention_route_takes(*shape) is True
    assert mx_attention._mxi_attention_route_takes(3, 5, 77, 192, 64) is False
