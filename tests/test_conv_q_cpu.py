"""Converted per-tensor int8 convolutions without a GPU: the C ABI's new entry points and their host-side declines, the graph pass's
third branch (aten.conv2d -> conv2d_q) bit for bit against the unfused graph with every case it must leave alone, the router's
eligibility predicate reason by reason, and the committed route rule on the rows of profiles/conv2d_q.txt."""
import ctypes
import os
import re

import pytest
import torch

from quantized_training import _native, mx_operand, pt2e_native
from quantized_training import quantize_pt2e as qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["qt_q8_conv2d", "qt_quantize_codes_nhwc_bf16", "qt_quantize_codes_nhwc_f32"]
Q, DQ, CONV, LIN = ("quantized_ops.quantize.default", "quantized_ops.dequantize.default", "aten.conv2d.default", "aten.linear.default")
CONV_Q, LIN_Q = "quantized_ops.conv2d_q.default", "quantized_ops.linear_q.default"
SPEC = "int8,qs=per_tensor_symmetric"


# ---- symbols and host-side declines -----------------------------------------------------------------------------------------------------
def test_entry_points_are_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    cdll = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint\s+" + name + r"\(([^;]*?)\);", header, re.S)
        assert decl is not None, name
        assert name in _native.SIGNATURES, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(_native.SIGNATURES[name][1]), name
        getattr(cdll, name)


def _aligned(nbytes=4096):
    buf = ctypes.create_string_buffer(nbytes + 16)
    p = ctypes.addressof(buf)
    return buf, p + (-p) % 16


def test_q8_conv2d_answers_its_declines_before_any_device_call():
    L = _native.lib()
    keep, p = _aligned()

    def call(x=p, w=p, y=p, bias=None, s=None, n=1, h=4, wd=4, cin=32, cout=8, kh=1, kw=1, sh=1, ph=0, dh=1):
        return L.qt_q8_conv2d(x, w, y, 1, bias, s, 0, 0, n, h, wd, cin, cout, kh, kw, sh, sh, ph, ph, dh, dh, None)
    BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED
    assert call(x=None) == BAD and call(w=None) == BAD and call(y=None) == BAD
    assert [call(cin=c) for c in (0, 16, 48, 33)] == [BAD] * 4                      # Cin 16 is NOT admitted
    assert call(cin=1 << 15, kh=2, kw=2) == BAD and call(cin=32, kh=64, kw=64, h=64, wd=64) == BAD       # kh kw Cin = 2^17
    assert call(cin=(1 << 17) - 32, cout=0) == 0                                   # 2^17 - 32 passes the limit (empty output: no launch)
    assert call(sh=0) == BAD and call(dh=0) == BAD and call(ph=-1) == BAD and call(kh=0) == BAD and call(h=0) == BAD and call(n=-1) == BAD
    assert call(n=1 << 20, h=1 << 10, wd=1 << 10) == BAD                           # N Ho Wo >= 2^31
    assert call(ph=1 << 20, h=1 << 21) == BAD
    assert call(x=p + 1) == UNAL and call(w=p + 8) == UNAL and call(y=p + 4) == UNAL and call(bias=p + 4) == UNAL and call(s=p + 2) == UNAL
    assert call(n=0) == 0 and call(cout=0) == 0 and call(h=2, wd=2, kh=3, kw=3) == 0
    assert call(n=0, x=p + 1) == 0                                                 # nothing to read: alignment does not matter
    del keep


def test_codes_kernel_answers_its_declines_before_any_device_call():
    L = _native.lib()
    keep, p = _aligned()
    fmt = _native.QtFormat(_native.QT_FMT_LUT, 0, 0, 0.0, 0.0)
    BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED
    for fn in (L.qt_quantize_codes_nhwc_bf16, L.qt_quantize_codes_nhwc_f32):
        def call(x=p, codes=p, n=2, hw=16, c=32, strides=(512, 1, 16), f=ctypes.byref(fmt), lut=p, s=p):
            return fn(x, codes, n, hw, c, *strides, f, lut, s, None)
        assert call(x=None) == BAD and call(codes=None) == BAD and call(s=None) == BAD and call(f=None) == BAD and call(lut=None) == BAD
        assert call(c=24, strides=(384, 1, 16)) == BAD and call(strides=(1024, 1, 16)) == BAD and call(strides=(512, 2, 16)) == BAD
        assert call(n=65536) == BAD and call(n=-1) == BAD
        assert call(x=p + 4) == UNAL and call(codes=p + 1) == UNAL
        assert call(n=0) == 0 and call(hw=0, strides=(0, 1, 0)) == 0
    del keep


# ---- the graph pass -------------------------------------------------------------------------------------------------------------------
class SmallCnn(torch.nn.Module):
    """A stem over 3 channels, two 3 x 3 convolutions at 32 / 64 channels, a residual add, a Linear head."""

    def __init__(self):
        super().__init__()
        self.stem = torch.nn.Conv2d(3, 32, 3, padding=1)
        self.c1 = torch.nn.Conv2d(32, 64, 3, padding=1, stride=2)
        self.c2 = torch.nn.Conv2d(64, 64, 3, padding=1)
        self.fc = torch.nn.Linear(64, 10)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.c1(x))
        x = torch.relu(self.c2(x)) + x
        return self.fc(x.mean((2, 3)))


class OneConv(torch.nn.Module):
    def __init__(self, **kw):
        super().__init__()
        self.conv = torch.nn.Conv2d(32, 16, 3, **kw)

    def forward(self, x):
        return self.conv(x)


def convert(net, x, dtype=torch.float32):
    torch.manual_seed(1)
    net = net.to(dtype).eval()
    gm = qp.prepare_pt2e(net, qp.get_default_quantizer(SPEC, None, SPEC, "int24"), (x,))
    with torch.no_grad():
        gm(x), gm(x * 0.5)
    return qp.convert_pt2e(gm, native=False)


def rows(gm):
    return [(n.op, str(n.target), tuple(str(a) for a in n.args)) for n in gm.graph.nodes]


def calls(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


def node_of(gm, target, index=0):
    return [n for n in gm.graph.nodes if str(n.target) == target][index]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pass_rewrites_the_eligible_convolutions(dtype):
    torch.manual_seed(0)
    x = torch.randn(2, 3, 12, 12).to(dtype)
    gc = convert(SmallCnn(), x, dtype)
    before = calls(gc)
    assert before.count(CONV) == 3 and before.count(LIN) == 1 and before.count(Q) == 4 and before.count(DQ) == 4
    with torch.no_grad():
        y0 = gc(x)
    assert pt2e_native.fuse_native_gemms(gc) == 3                    # two convolutions and the Linear; the stem (Cin 3) stays
    after = calls(gc)
    assert after.count(CONV) == 1 and after.count(CONV_Q) == 2 and after.count(LIN_Q) == 1 and after.count(LIN) == 0
    # the stem keeps its quantize and dequantize; the quantize node shared by c2 and the residual add stays for the add
    assert after.count(Q) == 2 and after.count(DQ) == 1
    shared = [n for n in gc.graph.nodes if str(n.target) == Q and any(str(u.target) == "aten.add.Tensor" for u in n.users)]
    assert len(shared) == 1 and all(str(u.target) != CONV_Q for u in shared[0].users)
    c2 = node_of(gc, CONV_Q, 1)
    assert c2.args[0] is shared[0].args[0] and c2.args[1] is shared[0].args[1] and c2.args[2] is shared[0].args[5]
    c1 = node_of(gc, CONV_Q, 0)
    assert list(c1.args[5:9]) == [[2, 2], [1, 1], [1, 1], 1] and c1.args[11] == "int8"
    assert list(c2.args[5:9]) == [[1, 1], [1, 1], [1, 1], 1]
    assert tuple(gc.c1_weight_codes.shape) == (64, 3, 3, 32) and tuple(gc.c2_weight_codes.shape) == (64, 3, 3, 64)
    assert gc.c1_weight_codes.dtype == torch.int8 and gc.c1_weight_codes.is_contiguous()
    assert torch.equal(gc.c1_weight_codes.permute(0, 3, 1, 2).to(dtype), gc.get_parameter("c1.weight") if "c1.weight" in dict(gc.named_parameters())
                       else gc.get_buffer("c1.weight"))
    assert "c1_weight_codes" not in gc.state_dict()                 # non-persistent
    stored = dict(gc.named_parameters()).get("c1.weight")
    stored = stored if stored is not None else gc.get_buffer("c1.weight")
    assert pt2e_native._conv_weight_values(gc.c1_weight_codes, dtype).data_ptr() == stored.data_ptr()      # the fallback's values: no copy
    with torch.no_grad():
        y1 = gc(x)
    assert y1.dtype == y0.dtype and torch.equal(y1, y0)             # the CPU implementation is the three nodes verbatim
    snapshot = rows(gc)
    assert pt2e_native.fuse_native_gemms(gc) == 0 and rows(gc) == snapshot          # idempotent


def test_meta_implementation_infers_the_shape():
    x = torch.empty(2, 32, 9, 7, device="meta")
    wc = torch.empty(24, 3, 3, 32, dtype=torch.int8, device="meta")
    s = torch.empty((), device="meta")
    y = torch.ops.quantized_ops.conv2d_q(x, s, torch.empty(65536, dtype=torch.bfloat16, device="meta"), wc, None, [2, 1], [1, 2], [1, 2], 1,
                                         s, None, "int8")
    assert y.shape == (2, 24, 5, 7) and y.device.type == "meta"


def _one_conv(**kw):
    torch.manual_seed(0)
    x = torch.randn(2, 32, 8, 8)
    return convert(OneConv(**kw), x), x


def _plain_then_copy(**kw):
    """The positive control of a decline test: an untouched copy of the layer fuses.  Returns a second, identical conversion for the
    test to mutate, so that what keeps it unfused is the mutation."""
    control, _ = _one_conv(**kw)
    assert pt2e_native.fuse_native_gemms(control) == 1 and calls(control).count(CONV_Q) == 1
    return _one_conv(**kw)


def _assert_untouched(gc, x):
    snapshot = rows(gc)
    with torch.no_grad():
        y0 = gc(x)
    assert pt2e_native.fuse_native_gemms(gc) == 0
    assert rows(gc) == snapshot and CONV_Q not in calls(gc)
    with torch.no_grad():
        assert torch.equal(gc(x), y0)


def test_pass_takes_the_plain_layer():
    gc, x = _one_conv(padding=1)
    with torch.no_grad():
        y0 = gc(x)
    assert pt2e_native.fuse_native_gemms(gc) == 1 and calls(gc).count(CONV_Q) == 1
    with torch.no_grad():
        assert torch.equal(gc(x), y0)


def test_pass_declines_a_per_channel_activation():
    gc, x = _plain_then_copy(padding=1)
    q = node_of(gc, Q)
    q.args = (*q.args[:3], [1], *q.args[4:])                         # axes given: not a per-tensor quantize
    snapshot = rows(gc)
    assert pt2e_native.fuse_native_gemms(gc) == 0 and rows(gc) == snapshot


def test_pass_declines_a_weight_that_is_not_int8():
    gc, x = _plain_then_copy(padding=1)
    w = node_of(gc, CONV).args[1]
    w.meta["dtype"] = "fp8_e4m3"
    _assert_untouched(gc, x)


@pytest.mark.parametrize("value", [0.5, 300.0])
def test_pass_declines_a_weight_value_that_is_no_int8_integer(value):
    gc, x = _plain_then_copy(padding=1)
    w = node_of(gc, CONV).args[1]
    t = dict(gc.named_parameters()).get(w.target)
    t = t if t is not None else gc.get_buffer(w.target)
    with torch.no_grad():
        t.view(-1)[5] = value
    _assert_untouched(gc, x)


def test_pass_declines_a_dequantize_with_a_non_identity_map():
    gc, x = _plain_then_copy(padding=1)
    dq = node_of(gc, DQ)
    assert dq.args[5] is not None
    mx_operand.tag_map(gc.get_buffer(dq.args[5].target), "int8")
    _assert_untouched(gc, x)


def test_pass_declines_a_dequantize_that_is_not_the_sole_user():
    gc, x = _plain_then_copy(padding=1)
    conv, dq = node_of(gc, CONV), node_of(gc, DQ)
    with gc.graph.inserting_after(dq):
        extra = gc.graph.call_function(torch.ops.aten.add.Tensor, (dq, conv))
    dq.replace_all_uses_with(extra, delete_user_cb=lambda u: u is not extra)
    gc.graph.lint()
    gc.recompile()
    _assert_untouched(gc, x)


def test_pass_declines_string_padding():
    _plain_then_copy(padding=1)
    gc, x = _one_conv(padding="same")                                  # exports as the string-padding overload of aten.conv2d
    conv = [n for n in gc.graph.nodes if str(n.target).startswith("aten.conv2d")]
    assert len(conv) == 1 and any(isinstance(a, str) for a in conv[0].args)
    _assert_untouched(gc, x)
    gc, x = _one_conv(padding=1)                                       # and a string where the default overload's padding belongs
    conv = node_of(gc, CONV)
    conv.args = (*conv.args[:4], "same", *conv.args[5:])
    snapshot = rows(gc)
    assert pt2e_native.fuse_native_gemms(gc) == 0 and rows(gc) == snapshot


def test_pass_declines_non_static_geometry():
    gc, x = _plain_then_copy(padding=1)
    conv = node_of(gc, CONV)
    assert pt2e_native._conv_args(conv) is not None
    conv.args = (*conv.args[:3], [conv.args[0], 1], *conv.args[4:])   # a graph node where a stride belongs
    assert pt2e_native._conv_args(conv) is None
    snapshot = rows(gc)
    assert pt2e_native.fuse_native_gemms(gc) == 0 and rows(gc) == snapshot


def test_conv_args_fills_in_the_defaults():
    g = torch.fx.Graph()
    x, w = g.placeholder("x"), g.placeholder("w")
    n = g.call_function(torch.ops.aten.conv2d.default, (x, w))
    assert pt2e_native._conv_args(n) == (x, w, None, [1, 1], [0, 0], [1, 1], 1)
    n = g.call_function(torch.ops.aten.conv2d.default, (x, w, None, 2, [3]), {"groups": 4})
    assert pt2e_native._conv_args(n) == (x, w, None, [2, 2], [3, 3], [1, 1], 4)
    assert pt2e_native._conv_args(g.call_function(torch.ops.aten.conv2d.default, (x, w, None, [1, 1], "same"))) is None


# ---- the router's eligibility predicate -----------------------------------------------------------------------------------------------
def _op_args(dtype=torch.bfloat16, cin=32, cout=16, k=(3, 3), h=8, w=8, n=2):
    x = torch.randn(n, cin, h, w).to(dtype)
    scale = torch.tensor(0.05).to(dtype)
    qmap = torch.zeros(65536, dtype=torch.bfloat16)
    wc = torch.zeros((cout, *k, cin), dtype=torch.int8)
    out_scale = torch.tensor([1e-3]).to(dtype)
    return dict(input=x, scale=scale, qmap=qmap, weight_codes=wc, bias=torch.zeros(cout, dtype=dtype), stride=[1, 1], padding=[1, 1],
                dilation=[1, 1], groups=1, out_scale=out_scale, kind="int8")


def _why(monkeypatch, on_device=True, rule=True, **change):
    monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", lambda *a: rule)
    a = _op_args(**{k: change.pop(k) for k in list(change) if k in ("dtype", "cin", "cout", "k", "h", "w", "n")})
    a.update(change)
    return pt2e_native._conv_q_decline(**a, on_device=on_device)


def test_router_takes_the_plain_call_and_names_every_decline(monkeypatch):
    assert _why(monkeypatch) is None
    assert _why(monkeypatch, dtype=torch.float32) is None
    assert _why(monkeypatch, on_device=None) == "not a device tensor"              # the real device test on a host tensor
    assert "kind" in _why(monkeypatch, kind="fp8_e4m3")
    assert "kind" in _why(monkeypatch, weight_codes=torch.zeros((16, 3, 3, 32), dtype=torch.uint8))
    assert "model dtype" in _why(monkeypatch, dtype=torch.float16)
    assert "input (" in _why(monkeypatch, input=torch.zeros(2, 32, 8))
    assert "input (" in _why(monkeypatch, n=0)
    assert _why(monkeypatch, groups=2) == "groups 2"
    for cin in (3, 16, 48):
        assert "not a multiple of 32" in _why(monkeypatch, cin=cin)
    assert "not a multiple of 32" in _why(monkeypatch, weight_codes=torch.zeros((16, 3, 3, 64), dtype=torch.int8))      # Cin of the weight differs
    assert ">= 2^17" in _why(monkeypatch, cin=1 << 14, k=(2, 4), h=2, w=4, n=1, cout=1, padding=[0, 0])
    assert _why(monkeypatch, cin=(1 << 14) - 32, k=(2, 4), h=2, w=4, n=1, cout=1, padding=[0, 0], bias=None) is None
    assert "value map" in _why(monkeypatch, qmap=torch.zeros(65536))
    assert "value map" in _why(monkeypatch, qmap=torch.zeros(256, dtype=torch.bfloat16))
    assert "activation scale" in _why(monkeypatch, scale=torch.tensor(0.05))                   # fp32 scale in a bf16 model
    assert "activation scale" in _why(monkeypatch, scale=torch.tensor([0.05, 0.05]).bfloat16())
    assert "dequantize scale" in _why(monkeypatch, out_scale=torch.ones(3).bfloat16())
    assert _why(monkeypatch, out_scale=torch.ones(16, 1, 1).bfloat16()) is None                # per output channel
    assert "bias" in _why(monkeypatch, bias=torch.zeros(3).bfloat16())
    assert "empty output" in _why(monkeypatch, h=2, w=2, padding=[0, 0])
    base = torch.zeros(2 * 32 * 8 * 8 + 8, dtype=torch.bfloat16)
    off = next(o for o in range(1, 8) if base[o:].data_ptr() % 16)
    assert _why(monkeypatch, input=base[off:off + 4096].view(2, 32, 8, 8)) == "misaligned operand"
    assert _why(monkeypatch, weight_codes=torch.zeros((16, 32, 3, 3), dtype=torch.int8).permute(0, 2, 3, 1)) == "misaligned operand"
    assert _why(monkeypatch, rule=False) == "route rule: profiles/conv2d_q.txt"
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    assert _why(monkeypatch, rule=False) is None


def test_operator_on_the_host_is_the_three_nodes(monkeypatch):
    from quantized_training.fake_quantize import get_quantization_map
    torch.manual_seed(0)
    a = _op_args(dtype=torch.float32)
    a["qmap"] = get_quantization_map("int8")
    a["weight_codes"] = torch.randint(-127, 128, a["weight_codes"].shape).to(torch.int8)
    a["bias"] = torch.randint(-100, 100, (16,)).float()
    before = dict(pt2e_native.STATS)
    y = torch.ops.quantized_ops.conv2d_q(a["input"], a["scale"], a["qmap"], a["weight_codes"], a["bias"], [1, 1], [1, 1], [1, 1], 1,
                                         a["out_scale"], None, "int8")
    xq = torch.ops.quantized_ops.quantize(a["input"], a["scale"], None, None, None, a["qmap"])
    want = torch.ops.quantized_ops.dequantize(
        torch.nn.functional.conv2d(xq, a["weight_codes"].permute(0, 3, 1, 2).float().contiguous(), a["bias"], 1, 1), a["out_scale"],
        None, None, None, None)
    assert torch.equal(y, want) and dict(pt2e_native.STATS) == before


# ---- the committed rule ---------------------------------------------------------------------------------------------------------------
def _profile_rows():
    """(m, cin, cout, k, clears the bar) of every row of profiles/conv2d_q.txt."""
    out = []
    for line in open(os.path.join(ROOT, "profiles", "conv2d_q.txt")):
        m = re.match(r"(\d+)x(\d+)x(\d+)x(\d+) -> (\d+) (\d+)x(\d+) \|.*clears the bar: (yes|no)", line)
        if m:
            n, cin, h, w, cout, kh, kw = (int(v) for v in m.groups()[:7])
            out.append((n * h * w, cin, cout, kh, kw, m.group(8) == "yes"))
    return out


def test_route_rule_follows_the_committed_table():
    table = _profile_rows()
    assert len(table) == 18                                          # ResNet-50's thirteen body layers and five smaller problems
    listed = 0
    for m, cin, cout, kh, kw, clears in table:
        takes = pt2e_native._conv_q_route_takes(m, cout, cin, kh, kw)
        assert isinstance(takes, bool)
        assert not takes or clears, f"the rule lists {m} x {cout} x {cin} {kh}x{kw}, which did not clear the bar"
        listed += takes
    assert listed == 10                                              # 3 x 3 / 7 x 7 over enough tiles, expanding 1 x 1
    # the classes by name: reducing 1 x 1 layers and problems of a few tiles stay with the graph
    assert pt2e_native._conv_q_route_takes(32 * 56 * 56, 64, 64, 3, 3) and pt2e_native._conv_q_route_takes(32 * 7 * 7, 2048, 512, 1, 1)
    assert not pt2e_native._conv_q_route_takes(32 * 7 * 7, 512, 2048, 1, 1) and not pt2e_native._conv_q_route_takes(196, 512, 512, 3, 3)
    # a fixed function of the shape: the same answer again
    assert [pt2e_native._conv_q_route_takes(m, co, ci, kh, kw) for m, ci, co, kh, kw, _ in table] == \
        [pt2e_native._conv_q_route_takes(m, co, ci, kh, kw) for m, ci, co, kh, kw, _ in table]
