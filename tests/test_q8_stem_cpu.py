"""The stem convolution of converted per-tensor int8 CNNs without a GPU: the new entry points and their host-side refusals, the graph
pass with and without stem=True, the mark, the router's reasons, and the committed rule on the rows of profiles/conv2d_q_stem.txt."""
import ctypes
import os
import re

import pytest
import torch

import conv_q_depthwise_cases as K
from quantized_training import _native, pt2e_native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, UNAL = _native.QT_ERR_BAD_ARG, _native.QT_ERR_UNALIGNED


@pytest.mark.parametrize("name,nargs", [("qt_q8_stem_conv2d", 22), ("qt_q8_stem_conv2d_codes", 27), ("qt_quantize_codes_nhwc4_bf16", 12),
                                        ("qt_quantize_codes_nhwc4_f32", 12)])
def test_entry_points_are_in_the_header_the_binding_and_the_library(name, nargs):
    header = open(os.path.join(ROOT, "include", "qt_hip.h")).read()
    decl = re.search(r"\bint\s+" + name + r"\(([^;]*?)\);", header, re.S)
    assert decl is not None and len([a for a in decl.group(1).split(",") if a.strip()]) == len(_native.SIGNATURES[name][1]) == nargs
    getattr(ctypes.CDLL(_native.LIB_PATH), name)
    assert _native.lib().qt_abi_version() == 3 and "1 <= Cin <= 4" in header and pt2e_native.STATS["conv2d_stem_int8"] >= 0


def check_refusals(L, p, stream):
    """Every refusal of the two stem entries and of the nhwc4 pass, with `p` a 16-byte aligned pointer to 64 KiB (host or device)."""
    def call(x=p, w=p, y=p, bias=None, s=None, n=1, h=20, wd=20, cin=3, cout=16, kh=3, kw=3, sh=1, sw=1, ph=0, pw=0, dh=1, dw=1):
        return L.qt_q8_stem_conv2d(x, w, y, 1, bias, s, 0, 0, n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, dh, dw, stream)
    assert [call(cin=v) for v in (0, 5, 32, -1)] == [BAD] * 4 and [call(cin=v, n=0) for v in (1, 2, 3, 4)] == [0] * 4
    assert [call(cout=v) for v in (8, 24, -16)] == [BAD] * 3 and call(cout=0) == 0
    assert call(kh=17, h=32) == BAD and call(kw=17, wd=32) == BAD and call(kh=16, kw=16, n=0) == 0
    assert call(dh=2) == BAD and call(dw=2) == BAD and call(dh=0) == BAD and call(sh=0) == BAD and call(sw=0) == BAD
    assert call(sh=4096) == BAD and call(sw=4096) == BAD                                    # the halo's LDS
    assert call(x=None) == BAD and call(w=None) == BAD and call(y=None) == BAD and call(h=0) == BAD and call(n=-1) == BAD and call(ph=-1) == BAD
    assert call(n=1 << 12, h=1 << 10, wd=1 << 10) == BAD                                    # 2^34 bytes of pixel dwords
    assert call(x=p + 4) == UNAL and call(w=p + 1) == UNAL and call(y=p + 8) == UNAL and call(bias=p + 4) == UNAL and call(s=p + 2) == UNAL
    assert call(n=0) == 0 and call(h=2, wd=2) == 0 and call(n=0, x=p + 1) == 0

    def codes(act=1, lo=0.0, hi=6.0, s=p, m=p, cout=16):
        return L.qt_q8_stem_conv2d_codes(p, p, p, 1, None, None, 0, 0, 1, 20, 20, 3, cout, 3, 3, 1, 1, 0, 0, 1, 1, act, lo, hi, s, m, stream)
    assert codes(act=2) == BAD and codes(lo=7.0) == BAD and codes(hi=float("nan")) == BAD and codes(s=None) == BAD and codes(m=None) == BAD
    assert codes(s=p + 2) == UNAL and codes(m=p + 1) == UNAL and codes(cout=24) == BAD
    fmt = __import__("quantized_training.decomposed", fromlist=["_lut_format"])._lut_format()

    def pass4(x=p, y=p, n=2, hw=64, c=3, bs=192, rs=1, cs=64, lut=p, scale=p, f=ctypes.byref(fmt)):
        return L.qt_quantize_codes_nhwc4_bf16(x, y, n, hw, c, bs, rs, cs, f, lut, scale, stream)
    assert pass4(c=5) == BAD and pass4(c=-1) == BAD and pass4(rs=2) == BAD and pass4(cs=32) == BAD and pass4(bs=191) == BAD
    assert pass4(x=None) == BAD and pass4(y=None) == BAD and pass4(scale=None) == BAD and pass4(lut=None) == BAD and pass4(f=None) == BAD
    assert pass4(n=1 << 20, hw=1 << 20, bs=3 << 20, cs=1 << 20) == BAD
    assert pass4(x=p + 2) == UNAL and pass4(y=p + 4) == UNAL and pass4(c=0) == 0 and pass4(n=0) == 0


def test_refusals_are_answered_before_any_device_call():
    buf = ctypes.create_string_buffer((1 << 16) + 16)
    check_refusals(_native.lib(), ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, None)


def targets(gm):
    return [str(n.target) for n in gm.graph.nodes if n.op == "call_function"]


def test_the_pass_takes_the_stem_only_when_asked():
    g0, _ = K.convert_block(torch.bfloat16, native=True)
    assert targets(g0).count("aten.conv2d.default") == 1 and not hasattr(g0, "stem_weight_codes")
    g1, _ = K.convert_block(torch.bfloat16, native=False)
    assert pt2e_native.fuse_native_gemms(g1, stem=True) == 4 and "aten.conv2d.default" not in targets(g1)
    codes = g1.stem_weight_codes
    assert tuple(codes.shape) == (16, 3, 3, 3) and pt2e_native._stem_marked(codes) and not pt2e_native._stem_marked(g1.expand_weight_codes)
    assert not pt2e_native._stem_marked(codes.clone()) and not pt2e_native._split_k_marked(codes)         # the mark is lost on copy


def test_decline_reasons(monkeypatch):
    qmap = torch.zeros(65536, dtype=torch.bfloat16)
    s, out_scale = torch.tensor(0.1, dtype=torch.bfloat16), torch.ones(1, dtype=torch.bfloat16)

    def why(cin=3, cout=32, k=(3, 3), stride=(2, 2), dilation=(1, 1), marked=True, hw=224, n=32, wcin=None):
        x = pt2e_native._Operand((n, cin, hw, hw), torch.bfloat16, "cpu")
        w = torch.zeros(cout, *k, cin if wcin is None else wcin, dtype=torch.int8)
        return pt2e_native._conv_q_decline(x, s, qmap, pt2e_native.mark_stem(w) if marked else w, None, list(stride), [1, 1], list(dilation), 1,
                                           out_scale, "int8", on_device=True)
    assert why() is None and why(cin=1) is None and why(cin=4, cout=64, k=(7, 7)) is None
    assert why(marked=False) == "Cin = 3 / 3: not a multiple of 32" and why(cin=5) == "Cin = 5 / 5: not a multiple of 32"
    assert why(n=1) == "stem route rule: profiles/conv2d_q_stem.txt" and why(cout=128) == "stem route rule: profiles/conv2d_q_stem.txt"
    monkeypatch.setattr(pt2e_native, "_APPLY_CONV_Q_RULE", False)
    assert why(n=1) is None and why(cout=128) is None
    assert "Cout = 24" in why(cout=24) and "17 x 3" in why(k=(17, 3)) and "dilation" in why(dilation=(2, 2)) and "stem Cin = 3 / 2" == why(wcin=2)
    assert "LDS budget" in why(stride=(4096, 1)) and why(k=(16, 16), stride=(1, 1)) is None
    # what the operator computes of the kernel's LDS is what csrc/qt_q8_stem_conv.hip computes: 7 x 7 / 2 -> 64 and 3 x 3 / 2 -> 32
    assert pt2e_native._stem_lds_bytes(64, 7, 7, 2, 2) == 4 * 38 * 22 + 64 * 272 and pt2e_native._stem_lds_bytes(32, 3, 3, 2, 2, True) == 10240 + 32 * 80


def test_rule_agrees_with_every_row_of_the_committed_table():
    rows = [ln for ln in open(os.path.join(ROOT, "profiles", "conv2d_q_stem.txt")) if "rule ->" in ln]
    assert len(rows) == 5
    for ln in rows:
        k, stride, cout, n, hw = (int(v) for v in re.search(r"(\d+)x\d+/(\d+) -> (\d+) (\d+)x3x(\d+)x", ln).groups())
        ho = (hw + 2 * {3: 1, 7: 3, 11: 2}[k] - k) // stride + 1
        clears, rule = "clears the bar: yes" in ln, "rule -> native" in ln
        assert pt2e_native._conv_q_stem_route_takes(n * ho * ho, cout, 3, k, k, stride, stride) == rule == clears, ln
        ratios = [float(v) for v in re.findall(r"ratio (\d+\.\d+)", ln)]
        assert len(ratios) == 4 and (min(ratios) > 1.0) == clears
