"""Chained converted int8 convolutions without a GPU: the three codes-out entry points and their host-side declines, the graph pass
fuse_conv_q_chains on CPU-converted graphs (rewritten edges node by node, idempotence, every edge it must leave alone), the
convert_pt2e switch, and the chained graph against the un-chained one bit for bit through the operator's fallbacks."""
import ctypes
import os
import re

import pytest
import torch

import conv_q_chain_cases as C
import conv_q_depthwise_cases as K
from quantized_training import _native, pt2e_native
from quantized_training import quantize_pt2e as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, DQ, CONV = "quantized_ops.quantize.default", "quantized_ops.dequantize.default", "aten.conv2d.default"
CONV_Q, CONV_QC, RELU = "quantized_ops.conv2d_q.default", "quantized_ops.conv2d_qc.default", "aten.relu.default"
ENTRIES = {"qt_q8_conv2d_codes": ("qt_q8_conv2d", 27), "qt_q8_dwconv2d_codes": ("qt_q8_dwconv2d", 26), "qt_q8_gemm_codes": ("qt_q8_gemm", 20)}


# ---- the symbols and their host-side declines ---------------------------------------------------------------------------------------
def test_entry_points_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name, (sibling, nargs) in ENTRIES.items():
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl is not None and name in _native.SIGNATURES
        args = [a.strip() for a in decl.group(1).split(",") if a.strip()]
        assert len(args) == len(_native.SIGNATURES[name][1]) == nargs == len(_native.SIGNATURES[sibling][1]) + 5, name
        assert args[2] == "int8_t *y" and [a.split()[-1].lstrip("*") for a in args[-6:]] == ["act", "act_lo", "act_hi", "next_scale", "next_qmap", "stream"]
        assert _native.SIGNATURES[name][1][:-6] == _native.SIGNATURES[sibling][1][:-1]          # the sibling's leading arguments
        getattr(lib, name)
    assert _native.lib().qt_abi_version() == 3
    assert pt2e_native.STATS["conv2d_codes_in"] >= 0 and pt2e_native.STATS["conv2d_codes_out"] >= 0


def test_entry_points_answer_their_declines_before_any_device_call():
    L = _native.lib()
    buf = ctypes.create_string_buffer(1 << 18)
    p = ctypes.addressof(buf)
    p += (-p) % 16
    nan = float("nan")
    BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED

    def conv(y=p, c=32, n=1, act=1, lo=0.0, hi=6.0, s=p, m=p, x=p, f32=1):
        return L.qt_q8_conv2d_codes(x, p, y, f32, None, None, 0, 0, n, 4, 4, 32, c, 1, 1, 1, 1, 0, 0, 1, 1, act, lo, hi, s, m, None)

    def dwc(y=p, c=32, n=1, act=1, lo=0.0, hi=6.0, s=p, m=p, x=p, f32=1):
        return L.qt_q8_dwconv2d_codes(x, p, y, f32, None, None, 0, 0, n, 4, 4, c, 1, 1, 1, 1, 0, 0, 1, 1, act, lo, hi, s, m, None)

    def gemm(y=p, c=32, n=1, act=1, lo=0.0, hi=6.0, s=p, m=p, x=p, f32=1):
        return L.qt_q8_gemm_codes(x, p, y, f32, None, None, 0, 0, 1, 16 * n, c, 16, 0, 0, act, lo, hi, s, m, None)

    for call in (conv, dwc, gemm):
        assert [call(c=c, n=1) for c in (24, 8, 40)] == [BAD] * 3                  # whole 16-byte runs of codes only
        assert call(m=None) == BAD and call(s=None) == BAD and call(y=None) == BAD and call(x=None) == BAD
        assert call(act=2) == BAD and call(act=-1) == BAD
        assert call(lo=6.5) == BAD and call(lo=nan) == BAD and call(hi=nan) == BAD and call(lo=float("inf"), hi=float("-inf")) == BAD
        assert call(y=p + 8) == UNAL and call(y=p + 1) == UNAL and call(m=p + 1) == UNAL
        assert call(s=p + 2) == UNAL and call(s=p + 1, f32=0) == UNAL and call(x=p + 4) == UNAL
        assert call(n=0) == 0 and call(n=0, act=0, lo=7.0) == 0                    # empty: no launch
    del buf


@pytest.mark.parametrize("family", ["gather", "dw", "gemm"])
def test_expected_codes_of_the_exact_tier_are_not_vacuous(family):
    """The host reference alone, for every case the GPU tests launch: a saturated code, a zero, at least 32 distinct codes, and with a
    clamp both bounds binding (C.expectation asserts it; the GPU tests reuse these expectations)."""
    keys = {"gather": [(m, c) for m in C.GATHER_M for c in C.GATHER_COUT], "dw": [(c,) for c in C.DW],
            "gemm": [(k, n) for k in C.GEMM_K for n in C.GEMM_N]}[family]
    for key in keys:
        for setting in C.settings(big=key[0] in C.DW_BIG):
            e = C.expectation(family, key, *setting)
            assert e["codes"].dtype == torch.int8 and e["codes"].shape == e["ops"]["exact"].shape


# ---- the graph pass -----------------------------------------------------------------------------------------------------------------
def rows(gm):
    return [(n.op, str(n.target), tuple(str(a) for a in n.args)) for n in gm.graph.nodes]


def nodes_of(gm, target):
    return [n for n in gm.graph.nodes if str(n.target) == target]


@pytest.fixture
def no_rule(monkeypatch):
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("net_cls,bounds", [(K.Block, (0.0, None)), (C.Block6, (0.0, 6.0))], ids=["relu", "relu6"])
def test_pass_chains_the_inverted_residual_block(no_rule, dtype, net_cls, bounds):
    plain, x = K.convert_block(dtype, native=True, net=C.seeded(net_cls))
    gm, _ = K.convert_block(dtype, native=True, net=C.seeded(net_cls))
    act = RELU if net_cls is K.Block else "aten.hardtanh.default"
    assert C.call_targets(gm) == [Q, CONV, DQ, act, CONV_Q, act, CONV_Q, act, CONV_Q]
    expand0, dw0, project0 = nodes_of(gm, CONV_Q)
    handed = [(dw0.args[1], dw0.args[2]), (project0.args[1], project0.args[2])]
    assert pt2e_native.fuse_conv_q_chains(gm) == 2
    after = rows(gm)
    assert pt2e_native.fuse_conv_q_chains(gm) == 0 and rows(gm) == after                       # idempotent
    assert C.call_targets(gm) == [Q, CONV, DQ, act, CONV_QC, CONV_QC, CONV_QC]
    expand, dw, project = nodes_of(gm, CONV_QC)
    assert (expand, dw, project) == (expand0, dw0, project0)
    stem_act = nodes_of(gm, act)[0]
    assert expand.args[0] is stem_act and expand.args[1] is not None and expand.args[2] is not None      # values in
    assert tuple(expand.args[12:]) == (*bounds, *handed[0])                                    # codes out for the depthwise layer
    assert dw.args[0] is expand and dw.args[1] is None and dw.args[2] is None                  # codes in
    assert tuple(dw.args[12:]) == (*bounds, *handed[1])
    assert project.args[0] is dw and project.args[1] is None and project.args[2] is None and tuple(project.args[12:]) == (None,) * 4
    for a, b in zip((expand0, dw0, project0), nodes_of(plain, CONV_Q)):
        assert [str(v) for v in a.args[3:12]] == [str(v) for v in b.args[3:12]]                # weights, bias, geometry, factors: as they were
    order = {n: i for i, n in enumerate(gm.graph.nodes)}
    assert all(order[a] < order[n] for n in (expand, dw, project) for a in n.all_input_nodes)
    with torch.no_grad():
        want, got = plain(x), gm(x)
    assert got.dtype == want.dtype and torch.equal(got, want) and bool(got.float().isfinite().all())


class Two(torch.nn.Module):
    """conv_a (32 -> mid, 3 x 3) -> act -> conv_b (and conv_c) -> an optional tail over the result and the activation."""

    def __init__(self, mid=32, act=torch.relu, tail=None, siblings=False):
        super().__init__()
        self.a = torch.nn.Conv2d(32, mid, 3, padding=1)
        self.b = torch.nn.Conv2d(mid, 32, 3, padding=1)
        self.c = torch.nn.Conv2d(mid, 32, 1) if siblings else None
        self.act, self.tail = act, tail
        self.register_buffer("lo", torch.tensor(0.25))

    def forward(self, x):
        y = self.act(self.a(x)) if self.act is not torch.clamp else torch.clamp(self.a(x), min=self.lo)
        z = self.b(y)
        if self.c is not None:
            z = z + self.c(y)
        return self.tail(z, y) if self.tail is not None else z


def convert_two(dtype=torch.bfloat16, **kw):
    torch.manual_seed(5)
    x = torch.randn(2, 32, 8, 8)
    return K.convert_block(dtype, native=True, net=C.seeded(lambda: Two(**kw)), x=x)


def test_pass_hands_one_code_array_to_sibling_consumers(no_rule):
    """Two convolutions read the same activation and quantize it with the same scale and map nodes: the producer writes one code
    array, both take it; an edge per consumer."""
    plain, x = convert_two(siblings=True)
    gm, _ = convert_two(siblings=True)
    a, b, c = nodes_of(gm, CONV_Q)
    assert b.args[0] is c.args[0] and b.args[1] is c.args[1] and b.args[2] is c.args[2]
    assert pt2e_native.fuse_conv_q_chains(gm) == 2 and pt2e_native.fuse_conv_q_chains(gm) == 0
    a, b, c = nodes_of(gm, CONV_QC)
    assert b.args[:3] == (a, None, None) and c.args[:3] == (a, None, None) and a.args[12:14] == (0.0, None) and RELU not in C.call_targets(gm)
    with torch.no_grad():
        assert torch.equal(gm(x), plain(x))


def strip_vals(gm):
    for n in gm.graph.nodes:
        n.meta.pop("val", None)


def different_scales(gm):
    """Gives the second sibling consumer a scale node of its own."""
    b, c = nodes_of(gm, CONV_Q)[1:]
    gm.register_buffer("other_scale", gm.get_buffer(str(c.args[1].target)).clone())
    with gm.graph.inserting_before(c):
        own = gm.graph.get_attr("other_scale")
    c.args = (c.args[0], own, *c.args[2:])
    gm.graph.lint()
    gm.recompile()


LEFT_ALONE = {
    "residual_tail": dict(net=dict(tail=lambda z, y: z + y)),                       # the activation also feeds the add's quantize
    "graph_output": dict(net=dict(tail=lambda z, y: (z, y))),                       # ... and the graph output
    "pooled_tail": dict(net=dict(tail=lambda z, y: z + torch.nn.functional.avg_pool2d(y, 1))),
    "different_scales": dict(net=dict(siblings=True), edit=different_scales),
    "cout_24": dict(net=dict(mid=24)),                                               # no kernel takes the consumer: it stays aten.conv2d
    "gelu": dict(net=dict(act=torch.nn.functional.gelu)),
    "aten_relu6": dict(net=dict(act=torch.nn.functional.relu6)),                     # aten.relu6 is not on the list (nn.ReLU6 is hardtanh)
    "clamp_tensor_bound": dict(net=dict(act=torch.clamp)),
    "one_sided_clamp": dict(net=dict(act=lambda t: torch.clamp(t, min=0.5))),        # both bounds must be static numbers
    "unknown_shapes": dict(net=dict(), edit=strip_vals),
    "rule_declines": dict(net=dict(), rule=True),                                    # 2 x 8 x 8 pixels: a few tiles, the rule keeps the graph
}


@pytest.mark.parametrize("which", list(LEFT_ALONE))
def test_pass_leaves_the_edge_alone(monkeypatch, which):
    cfg = LEFT_ALONE[which]
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", cfg.get("rule", False))
    gm, x = convert_two(**cfg["net"])
    if "edit" in cfg:
        cfg["edit"](gm)
    assert C.call_targets(gm).count(CONV_Q) >= 1
    before = rows(gm)
    with torch.no_grad():
        want = gm(x)
    assert pt2e_native.fuse_conv_q_chains(gm) == 0
    assert rows(gm) == before and CONV_QC not in C.call_targets(gm)
    with torch.no_grad():
        got = gm(x)
    for g, w in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
        assert torch.equal(g, w)


def test_plain_two_layer_net_is_chained(no_rule):
    """The control of the cases above: the same network without any of their obstacles is rewritten, for relu, hardtanh and a
    two-sided clamp, with the bounds the node carries."""
    for act, bounds in ((torch.relu, (0.0, None)), (torch.nn.functional.hardtanh, (-1.0, 1.0)),
                        (lambda t: torch.clamp(t, -0.5, 2), (-0.5, 2.0)), (torch.nn.ReLU6(), (0.0, 6.0))):
        plain, x = convert_two(act=act)
        gm, _ = convert_two(act=act)
        assert pt2e_native.fuse_conv_q_chains(gm) == 1
        a, b = nodes_of(gm, CONV_QC)
        assert tuple(a.args[12:14]) == bounds and b.args[:3] == (a, None, None)
        with torch.no_grad():
            assert torch.equal(gm(x), plain(x))


# ---- the switch ---------------------------------------------------------------------------------------------------------------------
def prepared(dtype=torch.bfloat16):
    torch.manual_seed(3)
    x = torch.randn(2, 3, 12, 12).to(dtype)
    net = C.seeded(K.Block).to(dtype).eval()
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(K.SPEC, None, K.SPEC, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    return gm, x


def test_convert_pt2e_switch(no_rule):
    """chain_convs defaults to False and returns today's graph, target for target; True applies the pass behind native fusion and
    only there; the chained graph's output equals the un-chained one bit for bit through the fallbacks."""
    today = [Q, CONV, DQ, RELU, CONV_Q, RELU, CONV_Q, RELU, CONV_Q]
    gm, x = prepared()
    default = qp.convert_pt2e(gm, native=True)
    assert C.call_targets(default) == today
    gm, _ = prepared()
    assert C.call_targets(qp.convert_pt2e(gm, native=True, chain_convs=False)) == today
    gm, _ = prepared()
    upstream = C.call_targets(qp.convert_pt2e(gm, native=False, chain_convs=True))
    assert CONV_Q not in upstream and CONV_QC not in upstream and upstream.count(CONV) == 4
    gm, _ = prepared()
    chained = qp.convert_pt2e(gm, native=True, chain_convs=True)
    assert C.call_targets(chained) == [Q, CONV, DQ, RELU, CONV_QC, CONV_QC, CONV_QC]
    with torch.no_grad():
        assert torch.equal(chained(x), default(x))


# ---- the operator on the host ---------------------------------------------------------------------------------------------------------
def test_operator_rejects_inconsistent_arguments():
    qmap = C.int8_map()
    x = torch.zeros(1, 32, 4, 4, dtype=torch.bfloat16)
    codes = torch.zeros(1, 32, 4, 4, dtype=torch.int8)
    w = torch.zeros(32, 1, 1, 32, dtype=torch.int8)
    s = torch.tensor(1.0, dtype=torch.bfloat16)
    geometry = ([1, 1], [0, 0], [1, 1], 1, s.reshape(1))
    op = torch.ops.quantized_ops.conv2d_qc
    for bad in ((x, None, None, w, None, *geometry, None, "int8", None, None, None, None),          # values without a scale
                (codes, None, qmap, w, None, *geometry, None, "int8", None, None, None, None),      # codes with a map
                (x, s, qmap, w, None, *geometry, None, "int8", 0.0, None, None, None),              # bounds without codes out
                (x, s, qmap, w, None, *geometry, None, "int8", None, None, s, None),                # codes out without a map
                (x, s, qmap, w, None, *geometry, None, "int8", 2.0, 1.0, s, qmap)):                 # lo > hi
        with pytest.raises(ValueError):
            op(*bad)
    y = op(x, s, qmap, w, None, *geometry, None, "int8", None, None, None, None)                    # values in, values out: conv2d_q
    assert y.dtype == torch.bfloat16 and y.shape == (1, 32, 4, 4)
    fake = op(codes.to("meta"), None, None, w.to("meta"), None, *geometry[:4], s.reshape(1).to("meta"), None, "int8", 0.0, 6.0, s.to("meta"), qmap.to("meta"))
    assert fake.dtype == torch.int8 and fake.shape == (1, 32, 4, 4)
    fake = op(codes.to("meta"), None, None, w.to("meta"), None, *geometry[:4], s.reshape(1).to("meta"), None, "int8", None, None, None, None)
    assert fake.dtype == torch.bfloat16


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_operator_on_the_host_equals_the_reference_codes(dtype):
    """conv2d_qc on host tensors, codes in and codes out, against the host reference of the kernels' exact tier: the exact sums, the
    rounding chain, torch.clamp, quantize, narrowed."""
    ops = C.gather_operands(126, 48)
    n, h, w = C.GATHER_M[126]
    codes = ops["x"].view(n, h, w, 32).permute(0, 3, 1, 2)
    for act in C.ACTS:
        e = C.expectation("gather", (126, 48), dtype, False, True, act)
        lo, hi = e["bounds"] if e["bounds"] is not None else (None, None)
        assert not e["fold"]
        got = torch.ops.quantized_ops.conv2d_qc(codes, None, None, ops["w"], e["bias"], [2, 2], [1, 1], [1, 1], 1, e["s"].reshape(-1, 1, 1),
                                                None, "int8", lo, hi, e["next_scale"].reshape(()), C.int8_map())
        assert got.dtype == torch.int8 and got.shape == (n, 48, 7, 9) and got.is_contiguous(memory_format=torch.channels_last)
        bad = got.permute(0, 2, 3, 1).reshape(-1, 48) != e["codes"]
        # the host's aten.conv2d accumulates in fp32 where the kernel's sum is exact: a code may differ where a sum rounds
        print(f"{dtype} {act}: {int(bad.sum())} of {bad.numel()} codes differ from the exact reference")
        assert float(bad.float().mean()) < 0.02
