"""The block-scaled float attention core off the GPU: the symbol, the committed route rule, and the operator on CPU tensors of a float
recipe (the replaced nodes, bit for bit, behind convert_pt2e on an exported toy)."""
import os

import torch

from quantized_training import _native, mx_attention
from quantized_training import quantize_pt2e as qp
from test_attention_mxi_cpu import ToyAttention, targets

OPS = torch.ops.quantized_ops


def test_symbol_and_route_rule():
    assert "qt_attention_mxf" in _native.SIGNATURES and getattr(_native.lib(), "qt_attention_mxf")
    header = os.path.join(os.path.dirname(__file__), "..", "include", "qt_hip.h")
    assert "int qt_attention_mxf(" in open(header).read() and _native.lib().qt_abi_version() == 3
    for shape, takes in mx_attention._MXF_ATTENTION_TABLE.items():      # the rule is the committed table
        assert takes is True and mx_attention._mxf_attention_route_takes(*shape) is True
    assert mx_attention._mxf_attention_route_takes(3, 5, 77, 384, 64) is False


def converted_toy(x, mask, **convert_kw):
    """ToyAttention exported, prepared with a float recipe's matmul quantizers (fp8_e4m3, block 32, power-of-two scales), calibrated
    and converted."""
    spec = "fp8_e4m3,qs=microscaling,bs=32,ax=-1"
    quantizer = qp.get_default_quantizer(spec, weight=spec, force_scale_power_of_two=True)
    gm = qp.prepare_pt2e(ToyAttention().eval(), quantizer, (x, mask)).to(x.device)
    with torch.no_grad():
        gm(x, mask)
    return qp.convert_pt2e(gm, native=True, **convert_kw)


def test_operator_on_cpu_tensors_is_the_nodes():
    torch.manual_seed(1)
    x = torch.randn(1, 2, 128, 64).to(torch.bfloat16)
    mask = torch.zeros(1, 1, 128, 128, dtype=torch.bfloat16).masked_fill(torch.ones(128, 128).triu(1).bool(), float("-inf"))
    off, on = converted_toy(x, mask, fuse_attention=False), converted_toy(x, mask, fuse_attention=True)
    assert targets(on).count(OPS.attention_mx.default) == 2 and OPS.attention_mx.default not in targets(off)
    assert [n.args[11:15] for n in on.graph.nodes if n.target == OPS.attention_mx.default] == [(True, None, False, 32)] * 2
    before = dict(mx_attention.STATS)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(on(x, mask), off(x, mask)))
    assert mx_attention.STATS == before                                 # CPU tensors never reach the device route
