"""Converted per-tensor int8 depthwise and narrow pointwise convolutions without a GPU: the new entry point qt_q8_dwconv2d and its host-side
declines, the graph pass on a converted inverted-residual block and on everything it must leave alone, the router's new reasons, the two
new route rules on the rows of profiles/conv2d_q_depthwise.txt, and the three nodes of a depthwise layer on the host against the stated
rounding chain."""
import ctypes
import os
import re

import pytest
import torch

import conv_q_depthwise_cases as K
from quantized_training import _native, mx_operand, pt2e_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, DQ, CONV = "quantized_ops.quantize.default", "quantized_ops.dequantize.default", "aten.conv2d.default"
CONV_Q = "quantized_ops.conv2d_q.default"
PROFILE = "profiles/conv2d_q_depthwise.txt"


# ---- the symbol and its host-side declines -------------------------------------------------------------------------------------------------
def test_entry_point_is_in_the_header_the_binding_and_the_library():
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    decl = re.search(r"\bint\s+qt_q8_dwconv2d\(([^;]*?)\);", header, re.S)
    assert decl is not None and "qt_q8_dwconv2d" in _native.SIGNATURES
    assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(_native.SIGNATURES["qt_q8_dwconv2d"][1]) == 21
    getattr(ctypes.CDLL(_native.LIB_PATH), "qt_q8_dwconv2d")
    assert _native.lib().qt_abi_version() == 3
    assert pt2e_native.STATS["conv2d_dw_int8"] >= 0 and "conv2d_int8" in pt2e_native.STATS


def test_q8_dwconv2d_answers_its_declines_before_any_device_call():
    L = _native.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.addressof(buf)
    p += (-p) % 16

    def call(x=p, w=p, y=p, bias=None, s=None, n=1, h=4, wd=4, c=16, kh=1, kw=1, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1):
        return L.qt_q8_dwconv2d(x, w, y, 1, bias, s, 0, 0, n, h, wd, c, kh, kw, sh, sw, ph, pw, dh, dw, None)
    BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED
    assert call(x=None) == BAD and call(w=None) == BAD and call(y=None) == BAD
    assert [call(c=c) for c in (0, 8, 24, 33, -16)] == [BAD] * 5
    assert call(c=16, n=0) == 0 and call(c=48, n=0) == 0 and call(c=144, n=0) == 0          # multiples of 16 pass the channel test
    assert call(kh=32, kw=32, h=32, wd=32) == BAD and call(kh=1024, kw=1, h=1024) == BAD    # kh kw = 1024
    assert call(kh=31, kw=33, h=31, wd=33, n=0) == 0                                        # 1023 passes the limit (empty: no launch)
    assert call(h=0) == BAD and call(wd=0) == BAD and call(n=-1) == BAD and call(kh=0) == BAD and call(kw=0) == BAD
    assert call(sh=0) == BAD and call(sw=0) == BAD and call(dh=0) == BAD and call(dw=0) == BAD and call(ph=-1) == BAD and call(pw=-1) == BAD
    assert call(n=1 << 20, h=1 << 10, wd=1 << 10) == BAD                                    # N Ho Wo >= 2^31
    assert call(n=1 << 10, h=1 << 10, wd=1 << 10, c=16) == BAD                              # N H W C = 2^34 bytes of codes
    assert call(ph=1 << 20, h=1 << 21) == BAD and call(sw=1 << 20) == BAD and call(kh=2, dh=1 << 19, h=1 << 21) == BAD
    assert call(x=p + 1) == UNAL and call(w=p + 8) == UNAL and call(y=p + 4) == UNAL and call(bias=p + 4) == UNAL and call(s=p + 2) == UNAL
    assert call(n=0) == 0 and call(h=2, wd=2, kh=3, kw=3) == 0 and call(h=4, wd=2, kh=1, kw=2, dw=2) == 0
    assert call(n=0, x=p + 1) == 0                                                          # nothing to read: alignment does not matter
    del buf


# ---- the graph pass ------------------------------------------------------------------------------------------------------------------------
def rows(gm):
    return [(n.op, str(n.target), tuple(str(a) for a in n.args)) for n in gm.graph.nodes]


def calls(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


def node_of(gm, target, index=0):
    return [n for n in gm.graph.nodes if str(n.target) == target][index]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pass_rewrites_the_inverted_residual_block(dtype):
    gc, x = K.convert_block(dtype)
    before = calls(gc)
    assert before.count(CONV) == 4 and before.count(Q) == 4 and before.count(DQ) == 4
    dw = node_of(gc, CONV, 2)
    assert list(dw.args[3:]) == [[2, 2], [1, 1], [1, 1], 96]          # the triple the pass matches, with groups = C
    with torch.no_grad():
        y0 = gc(x)
    assert pt2e_native.fuse_native_gemms(gc) == 3                     # expand, depthwise, project; the stem (Cin 3) stays
    after = calls(gc)
    assert after.count(CONV) == 1 and after.count(CONV_Q) == 3 and after.count(Q) == 1 and after.count(DQ) == 1
    assert node_of(gc, CONV).args[1].target == "stem.weight"
    expand, depthwise, project = (node_of(gc, CONV_Q, i) for i in range(3))
    assert list(expand.args[5:9]) == [[1, 1], [0, 0], [1, 1], 1] and list(project.args[5:9]) == [[1, 1], [0, 0], [1, 1], 1]
    assert list(depthwise.args[5:9]) == [[2, 2], [1, 1], [1, 1], 96] and depthwise.args[11] == "int8"
    for name, shape in (("dw_weight_codes", (96, 3, 3, 1)), ("expand_weight_codes", (96, 1, 1, 16)), ("project_weight_codes", (32, 1, 1, 96))):
        codes = getattr(gc, name)
        assert codes.dtype == torch.int8 and tuple(codes.shape) == shape and codes.is_contiguous() and name not in gc.state_dict()
    stored = dict(gc.named_parameters()).get("dw.weight")
    stored = stored if stored is not None else gc.get_buffer("dw.weight")
    assert torch.equal(gc.dw_weight_codes.permute(0, 3, 1, 2).to(dtype), stored)
    assert pt2e_native._conv_weight_values(gc.dw_weight_codes, dtype).data_ptr() == stored.data_ptr()       # the parameter itself: no copy
    with torch.no_grad():
        y1 = gc(x)
    assert y1.dtype == y0.dtype and torch.equal(y1, y0)               # on the host the operator is the three nodes verbatim
    snapshot = rows(gc)
    assert pt2e_native.fuse_native_gemms(gc) == 0 and rows(gc) == snapshot


def test_meta_implementation_infers_the_depthwise_shape():
    x = torch.empty(2, 96, 9, 7, device="meta")
    wc = torch.empty(96, 3, 3, 1, dtype=torch.int8, device="meta")
    s = torch.empty((), device="meta")
    y = torch.ops.quantized_ops.conv2d_q(x, s, torch.empty(65536, dtype=torch.bfloat16, device="meta"), wc, None, [2, 2], [1, 1], [1, 1], 96,
                                         s, None, "int8")
    assert y.shape == (2, 96, 5, 4) and y.device.type == "meta"


class OneConv(torch.nn.Module):
    def __init__(self, cin, cout, k, **kw):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, cout, k, **kw)

    def forward(self, x):
        return self.conv(x)


def _one(cin, cout, k, **kw):
    torch.manual_seed(0)
    return K.convert_block(torch.float32, net=OneConv(cin, cout, k, **kw), x=torch.randn(2, cin, 8, 8))


def _depthwise():
    return _one(32, 32, 3, padding=1, groups=32)


def _control_then_copy():
    """The positive control of a decline test: an untouched copy of the depthwise layer fuses; a second, identical conversion is
    returned for the test to mutate, so that what keeps it unfused is the mutation."""
    control, _ = _depthwise()
    assert pt2e_native.fuse_native_gemms(control) == 1 and calls(control).count(CONV_Q) == 1
    return _depthwise()


def _assert_untouched(gc, x):
    snapshot = rows(gc)
    with torch.no_grad():
        y0 = gc(x)
    assert pt2e_native.fuse_native_gemms(gc) == 0
    assert rows(gc) == snapshot and CONV_Q not in calls(gc)
    with torch.no_grad():
        assert torch.equal(gc(x), y0)


@pytest.mark.parametrize("cin,cout,k,kw", [
    (32, 32, 3, dict(padding=1, groups=2)),             # grouped, not depthwise (16 channels per group)
    (16, 32, 3, dict(padding=1, groups=16)),            # a depth multiplier of 2
    (24, 24, 3, dict(padding=1, groups=24)),            # depthwise over 24 channels
    (24, 32, 1, dict()),                                # pointwise over 24 channels
    (16, 32, 1, dict(stride=2)),                        # a strided 1 x 1 over 16 channels
    (16, 32, 1, dict(padding=1)),                       # a padded one
    (16, 32, 3, dict(padding=1)),                       # a 3 x 3 over 16 channels
], ids=["groups_2", "depth_multiplier", "depthwise_24", "pointwise_24", "strided_1x1", "padded_1x1", "3x3_over_16"])
def test_pass_leaves_alone(cin, cout, k, kw):
    gc, x = _one(cin, cout, k, **kw)
    assert calls(gc).count(CONV) == 1
    _assert_untouched(gc, x)


def test_pass_takes_the_narrow_pointwise_layers():
    for cin in (16, 48, 144):
        gc, x = _one(cin, 24, 1)
        with torch.no_grad():
            y0 = gc(x)
        assert pt2e_native.fuse_native_gemms(gc) == 1 and tuple(gc.conv_weight_codes.shape) == (24, 1, 1, cin)
        with torch.no_grad():
            assert torch.equal(gc(x), y0)


def test_pass_declines_a_depthwise_weight_that_is_not_int8():
    gc, x = _control_then_copy()
    node_of(gc, CONV).args[1].meta["dtype"] = "fp8_e4m3"
    _assert_untouched(gc, x)


def test_pass_declines_a_depthwise_weight_value_that_is_no_int8_integer():
    gc, x = _control_then_copy()
    w = node_of(gc, CONV).args[1]
    t = dict(gc.named_parameters()).get(w.target)
    t = t if t is not None else gc.get_buffer(w.target)
    with torch.no_grad():
        t.view(-1)[5] = 0.5
    _assert_untouched(gc, x)


def test_pass_declines_a_depthwise_dequantize_with_a_non_identity_map():
    gc, x = _control_then_copy()
    dq = node_of(gc, DQ)
    assert dq.args[5] is not None
    mx_operand.tag_map(gc.get_buffer(dq.args[5].target), "int8")
    _assert_untouched(gc, x)


def test_pass_declines_a_depthwise_dequantize_that_is_not_the_sole_user():
    gc, x = _control_then_copy()
    conv, dq = node_of(gc, CONV), node_of(gc, DQ)
    with gc.graph.inserting_after(dq):
        extra = gc.graph.call_function(torch.ops.aten.add.Tensor, (dq, conv))
    dq.replace_all_uses_with(extra, delete_user_cb=lambda u: u is not extra)
    gc.graph.lint()
    gc.recompile()
    _assert_untouched(gc, x)


def test_pass_declines_depthwise_string_padding():
    _control_then_copy()
    gc, x = _one(32, 32, 3, padding="same", groups=32)
    conv = [n for n in gc.graph.nodes if str(n.target).startswith("aten.conv2d")]
    assert len(conv) == 1 and any(isinstance(a, str) for a in conv[0].args)
    _assert_untouched(gc, x)


# ---- the router's predicate ------------------------------------------------------------------------------------------------------------------
def _args(dtype=torch.bfloat16, c=32, cout=None, k=(3, 3), h=8, w=8, n=2, groups=None, wcin=1):
    cout = c if cout is None else cout
    return dict(input=torch.randn(n, c, h, w).to(dtype), scale=torch.tensor(0.05).to(dtype), qmap=torch.zeros(65536, dtype=torch.bfloat16),
                weight_codes=torch.zeros((cout, *k, wcin), dtype=torch.int8), bias=torch.zeros(cout, dtype=dtype), stride=[1, 1],
                padding=[1, 1], dilation=[1, 1], groups=c if groups is None else groups, out_scale=torch.tensor([1e-3]).to(dtype), kind="int8")


def _why(monkeypatch, dw_rule=True, pw_rule=True, **change):
    monkeypatch.setattr(pt2e_native, "_conv_q_dw_route_takes", lambda *a: dw_rule)
    monkeypatch.setattr(pt2e_native, "_conv_q_pw16_route_takes", lambda *a: pw_rule)
    monkeypatch.setattr(pt2e_native, "_conv_q_route_takes", lambda *a: True)
    keys = ("dtype", "c", "cout", "k", "h", "w", "n", "groups", "wcin")
    a = _args(**{k: change.pop(k) for k in list(change) if k in keys})
    a.update(change)
    return pt2e_native._conv_q_decline(**a, on_device=True)


def test_router_takes_depthwise_calls_and_names_every_new_decline(monkeypatch):
    assert _why(monkeypatch) is None and _why(monkeypatch, dtype=torch.float32) is None
    assert _why(monkeypatch, c=16) is None and _why(monkeypatch, c=144, k=(5, 5), padding=[2, 2]) is None
    assert _why(monkeypatch, out_scale=torch.ones(32, 1, 1).bfloat16()) is None
    # every other grouped call answers exactly as before
    assert _why(monkeypatch, c=32, groups=2, wcin=16) == "groups 2"
    assert _why(monkeypatch, c=16, cout=32, groups=16) == "groups 16"                            # a depth multiplier of 2
    assert _why(monkeypatch, c=32, groups=32, wcin=2) == "groups 32"
    assert _why(monkeypatch, c=24) == "depthwise C = 24: not a multiple of 16"
    assert _why(monkeypatch, c=8) == "depthwise C = 8: not a multiple of 16"
    assert _why(monkeypatch, c=16, k=(32, 32), h=32, w=32, n=1, padding=[0, 0]) == "depthwise kh kw = 1024 > 1023"
    assert _why(monkeypatch, c=16, k=(31, 33), h=31, w=33, n=1, padding=[0, 0]) is None
    assert "model dtype" in _why(monkeypatch, dtype=torch.float16)
    assert "kind" in _why(monkeypatch, weight_codes=torch.zeros((32, 3, 3, 1), dtype=torch.uint8))
    assert "value map" in _why(monkeypatch, qmap=torch.zeros(65536))
    assert "activation scale" in _why(monkeypatch, scale=torch.tensor(0.05))
    assert "dequantize scale" in _why(monkeypatch, out_scale=torch.ones(3).bfloat16())
    assert "bias" in _why(monkeypatch, bias=torch.zeros(3).bfloat16())
    assert "empty output" in _why(monkeypatch, h=2, w=2, padding=[0, 0])
    base = torch.zeros(2 * 32 * 8 * 8 + 8, dtype=torch.bfloat16)
    off = next(o for o in range(1, 8) if base[o:].data_ptr() % 16)
    assert _why(monkeypatch, input=base[off:off + 4096].view(2, 32, 8, 8)) == "misaligned operand"
    assert _why(monkeypatch, dw_rule=False) == f"depthwise route rule: {PROFILE}"
    # the pointwise route: 1 x 1, stride 1, no padding, Cin = 16 mod 32
    pw = dict(groups=1, k=(1, 1), padding=[0, 0], cout=24)
    for cin in (16, 48, 144):
        assert _why(monkeypatch, c=cin, wcin=cin, **pw) is None
        assert _why(monkeypatch, pw_rule=False, c=cin, wcin=cin, **pw) == f"pointwise route rule: {PROFILE}"
    assert "not a multiple of 32" in _why(monkeypatch, c=24, wcin=24, **pw)
    assert "not a multiple of 32" in _why(monkeypatch, c=16, wcin=16, **dict(pw, stride=[2, 2]))
    assert "not a multiple of 32" in _why(monkeypatch, c=16, wcin=16, **dict(pw, padding=[1, 1]))
    assert "not a multiple of 32" in _why(monkeypatch, c=16, wcin=16, groups=1, cout=24)         # a 3 x 3 over 16 channels
    assert "not a multiple of 32" in _why(monkeypatch, c=16, wcin=48, **pw)                       # Cin of the weight differs
    assert _why(monkeypatch, pw_rule=False, c=64, wcin=64, **pw) is None                          # Cin % 32 == 0 stays with the gather kernel
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    assert _why(monkeypatch, dw_rule=False) is None and _why(monkeypatch, pw_rule=False, c=16, wcin=16, **pw) is None


def test_route_of_a_call():
    r = pt2e_native._conv_q_route
    x = torch.zeros(1, 32, 4, 4)
    assert r(x, torch.zeros(32, 3, 3, 1, dtype=torch.int8), [1, 1], [1, 1], 32) == "depthwise"
    assert r(x, torch.zeros(64, 3, 3, 1, dtype=torch.int8), [1, 1], [1, 1], 32) is None
    assert r(x, torch.zeros(32, 3, 3, 16, dtype=torch.int8), [1, 1], [1, 1], 2) is None
    assert r(x, torch.zeros(8, 1, 1, 32, dtype=torch.int8), [1, 1], [0, 0], 1) == "gather"
    assert r(x[:, :16], torch.zeros(8, 1, 1, 16, dtype=torch.int8), [1, 1], [0, 0], 1) == "pointwise"
    assert r(x[:, :16], torch.zeros(8, 1, 1, 16, dtype=torch.int8), [2, 1], [0, 0], 1) == "gather"


# ---- the committed rules -----------------------------------------------------------------------------------------------------------------------
def _profile_rows():
    """Depthwise rows (m, c, kh, kw, sh, sw, clears) and pointwise rows (m, cin, cout, clears) of the committed table."""
    dw, pw = [], []
    for line in open(os.path.join(ROOT, PROFILE)):
        m = re.match(r"depthwise (\d+)x(\d+)x(\d+)x(\d+) (\d+)x(\d+) stride (\d+) \|.*clears the bar: (yes|no)", line)
        if m:
            n, c, h, w, kh, kw, s = (int(v) for v in m.groups()[:7])
            p = kh // 2
            dw.append((n * ((h + 2 * p - kh) // s + 1) * ((w + 2 * p - kw) // s + 1), c, kh, kw, s, s, m.group(8) == "yes"))
        m = re.match(r"pointwise (\d+)x(\d+)x(\d+)x(\d+) -> (\d+) \|.*clears the bar: (yes|no)", line)
        if m:
            n, cin, h, w, cout = (int(v) for v in m.groups()[:5])
            pw.append((n * h * w, cin, cout, m.group(6) == "yes"))
    return dw, pw


def test_route_rules_follow_the_committed_table():
    dw, pw = _profile_rows()
    assert len(dw) == 13 and len(pw) == 3           # MobileNetV2's ten depthwise shapes, a 5 x 5 layer, two batch-4 problems; three pointwise layers
    for m, c, kh, kw, sh, sw, clears in dw:
        takes = pt2e_native._conv_q_dw_route_takes(m, c, kh, kw, sh, sw)
        assert isinstance(takes, bool)
        assert not takes or clears, f"the depthwise rule lists {m} x {c} {kh}x{kw} stride {sh}, which did not clear the bar"
        assert takes == pt2e_native._conv_q_dw_route_takes(m, c, kh, kw, sh, sw)
    for m, cin, cout, clears in pw:
        takes = pt2e_native._conv_q_pw16_route_takes(m, cout, cin)
        assert isinstance(takes, bool)
        assert not takes or clears, f"the pointwise rule lists {m} x {cout} x {cin}, which did not clear the bar"
    # a class is listed only where every one of its rows cleared the bar: a listed class has at least one row in the table
    assert DW_LISTED == sum(pt2e_native._conv_q_dw_route_takes(*r[:6]) for r in dw)
    assert PW_LISTED == sum(pt2e_native._conv_q_pw16_route_takes(m, cout, cin) for m, cin, cout, _ in pw)


DW_LISTED, PW_LISTED = 13, 3         # rows of the table the committed rules send to the native route: every row cleared the bar


def test_route_rules_keep_what_was_not_measured_with_the_graph():
    dw, pw = pt2e_native._conv_q_dw_route_takes, pt2e_native._conv_q_pw16_route_takes
    assert dw(32 * 56 * 56, 144, 3, 3, 1, 1) and dw(32 * 14 * 14, 240, 5, 5, 2, 2) and dw(4 * 14 * 14, 576, 3, 3, 1, 1)
    assert not dw(4 * 14 * 14, 560, 3, 3, 1, 1)             # fewer output elements than the smallest problem measured
    assert not dw(32 * 28 * 28, 32, 7, 7, 1, 1) and not dw(32 * 28 * 28, 192, 3, 3, 3, 3) and not dw(2 * 3 * 3, 96, 3, 3, 2, 2)
    assert pw(32 * 28 * 28, 32, 144) and pw(32 * 112 * 112, 96, 16) and pw(32 * 56 * 56, 24, 48)
    assert not pw(32 * 28 * 28 - 1, 32, 144) and not pw(32 * 28 * 28, 40, 240) and not pw(2 * 12 * 12, 96, 16)


# ---- the three nodes of a depthwise layer on the host are the stated chain ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [K.BF16, K.F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("case", K.FIRST_FIVE)
def test_three_nodes_on_the_host_equal_the_rounding_chain(case, per_channel, dtype):
    """quantize -> aten.conv2d(groups = C) -> dequantize on host tensors against round(round(float(sum) + bias) * s), no tolerance: every
    partial sum of the host's fp32 (or bf16-in, fp32-accumulate) convolution is an integer below 2^24, hence exact, so the only
    roundings are the chain's two."""
    n, h, w, c, (kh, kw), stride, padding, dilation = K.CASES[case]
    ops = K.operands(case)
    from quantized_training.fake_quantize import get_quantization_map
    qmap = get_quantization_map("int8")
    s_x = torch.tensor(0.25).to(dtype)
    x = (ops["xq"].float() * 0.25).to(dtype)                       # quantize gives the codes back: q = x / s exactly
    bias = ops["bias"].to(dtype)
    s = (ops["scale"] if per_channel else ops["scale"][:1]).to(dtype)
    xq = torch.ops.quantized_ops.quantize(x, s_x, None, None, None, qmap)
    assert torch.equal(xq.float(), ops["xq"].float())
    y = torch.nn.functional.conv2d(xq, ops["wq"].to(dtype), bias, stride, padding, dilation, c)
    got = torch.ops.quantized_ops.dequantize(y, s.view(-1, 1, 1) if per_channel else s, None, None, None, None)
    want = K.chain(ops["exact"], bias, s, dtype, 0)
    bits = torch.int16 if dtype == K.BF16 else torch.int32
    got = got.permute(0, 2, 3, 1).reshape(n, -1, c).contiguous()
    assert got.dtype == dtype and torch.equal(got.view(bits), want.contiguous().view(bits))
    # and through the operator on the host, which is those three nodes
    wc = ops["w"].reshape(c, kh, kw, 1)
    op = torch.ops.quantized_ops.conv2d_q(x, s_x, qmap, wc, bias, list(stride), list(padding), list(dilation), c,
                                          s.view(-1, 1, 1) if per_channel else s, None, "int8")
    assert torch.equal(op.permute(0, 2, 3, 1).reshape(n, -1, c).contiguous().view(bits), want.contiguous().view(bits))
